/*
 * mvbev.h — C ABI of the MI355X-native MVDet project+fuse hot path.
 *
 * libmvbev.so (built from the HIP sources in mvdet_amd/csrc for gfx950) exports exactly the
 * functions below.  Plain pointers and sizes only: every tensor argument is a
 * caller-owned DEVICE pointer (PyTorch caching allocator, hipMalloc, ...), every
 * call is enqueued on the caller's HIP stream (passed as `void*`, NULL = the
 * null stream), no call allocates, copies to the host or synchronises, and all
 * calls are reentrant (no global mutable state).
 *
 * Return value: 0 (MVBEV_OK) on success, a negative MVBEV_ERR_* code for a bad
 * argument (nothing is launched), or MVBEV_ERR_HIP when the launch itself
 * failed.  mvbev_status_string() turns a code into text.
 *
 * Reference interfaces replaced (ErikBrorsson/MVDet @ 2024-08-07):
 *   mvbev_warp_perspective_f32 / _f16
 *       kornia.geometry.transform.warp_perspective(img_feature, proj_mat,
 *       reducedgrid_shape)   multiview_detector/models/persp_trans_detector.py:69
 *       (kornia 0.6.11: normalize -> inverse -> meshgrid -> transform_points ->
 *       F.grid_sample(bilinear, zeros, align_corners=True)).  The caller passes
 *       the kornia src_norm<-dst_norm 3x3 (host-computed, same recipe) so the
 *       device does transform + divide + bilinear gather.  dst strides let every
 *       view write straight into its channel slice of the fused ground-plane
 *       tensor: the torch.cat at persp_trans_detector.py:77 becomes zero-copy.
 *   mvbev_fill_coord_map_f32
 *       self.coord_map.repeat([B,1,1,1]) concatenated as the last two channels
 *       (persp_trans_detector.py:21,77,103-112).
 *   mvbev_pack_conv3x3_weight_f32, mvbev_conv3x3_f32
 *       nn.Conv2d(Cin->Cout, 3, padding=d, dilation=d) (+ nn.ReLU) of
 *       map_classifier[0:4]   persp_trans_detector.py:51-53, :81; the conv1 contribution of
 *       the two constant coord channels plus its bias is input-independent and enters as
 *       the `init` term (once per weight version: mvbev_coord_term_f32, ABI 12300).
 *   mvbev_pack_conv3x3_weight_bf16x3, mvbev_conv3x3_bf16x3
 *       the same convs in 3xbf16 split precision on the bf16 MFMA (5.3x the fp32 rate)
 *   mvbev_conv3x3_cout1_f32
 *       nn.Conv2d(512->1, 3, padding=4, dilation=4, bias=False) of
 *       map_classifier[4]      persp_trans_detector.py:54, :81
 *   (the same-size F.interpolate at persp_trans_detector.py:82 is an exact
 *    identity and has no entry point.)
 */
#ifndef MVBEV_H_
#define MVBEV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVBEV_OK 0
#define MVBEV_ERR_RANK (-1)      /* a size is <= 0 / a rank assumption is violated */
#define MVBEV_ERR_SHAPE (-2)     /* inconsistent sizes (e.g. Cout not a multiple of 128) */
#define MVBEV_ERR_STRIDE (-3)    /* unsupported stride (innermost stride must be 1 where stated) */
#define MVBEV_ERR_ALIGN (-4)     /* pointer misaligned for the vector width used */
#define MVBEV_ERR_NULL (-5)      /* a required pointer is NULL */
#define MVBEV_ERR_DILATION (-6)  /* dilation not supported by this entry point */
#define MVBEV_ERR_HIP (-100)     /* the HIP launch failed (hipGetLastError) */

/* Input-channel granule of the conv kernels: packed K and every channel group must be
 * a multiple of this. */
#define MVBEV_CONV_KC 8
/* Output-channel granule of mvbev_conv3x3_f32. */
#define MVBEV_CONV_BN 128

const char* mvbev_status_string(int status);
/* Library / ABI version, e.g. 10000 for 1.0.0. */
int mvbev_version(void);  /* 12500: mvbev_bev_plan grew by params_nonfinite (rebuild callers); non-finite parameters raise the non-finite guard (mvbev_params_nonfinite_f32, mvbev_flag_raise, mvbev_bev_plan.params_nonfinite, mvbev_thin_conv1_forward_f32_ex, mvbev_thin_conv1_weight_mask), the exact path's map through :82's same-size interpolate (mvbev_conv3x3_cout1_f32_ex), the raise folded into the partials' reduce (mvbev_cout1_reduce_partials_ex), the training backward's gated direct data gradient (mvbev_pack_conv3x3_dgrad_bf16x3_gated, mvbev_mask_gated_u32), the parameter scan riding on the per-step pack and coord term (mvbev_pack_conv3x3_weight_wino_ex, mvbev_coord_term_f32_ex); 12400: row-Winograd F(4,3) (mvbev_pack_conv3x3_weight_wino43, mvbev_wino43_rows_split_bf16, mvbev_conv3x3_wino43_bf16x3, mvbev_conv3x3_wino43_bf16x3_cout1_partials); 12300: mvbev_coord_term_f32 (conv1's coord term as one VALU pass); 12200: the training forward's non-finite guard (mvbev_store_gated_f32, mvbev_pack_conv3x3_weight_f32_gated, mvbev_wino_rows_split_bf16_gated), per-geometry staging boxes of the fused warps (mvbev_warp_wino_boxes, mvbev_warp_views_wino_rows_ex, mvbev_warp_upsampled_wino_boxes, mvbev_warp_views_upsampled_wino_rows_ex); 12100: MVBEV_LAYOUT_SPLIT_BF16_PIX (conv data gradients' output, the warp adjoint's input); 12000: conv1's and conv2's weight gradients from the forward's row-Winograd transforms (mvbev_wino_dy_rows_f32, mvbev_conv3x3_wgrad_wino_bf16x3); 11900: row windows (mvbev_warp_views_split_bf16_rows with the non-finite report, mvbev_warp_views_exact_rows with fp16 sources), mvbev_conv3x3_f32_ex (row-band output), mvbev_bias_relu_nonfinite_f32, mvbev_zero_gated — the non-finite guard of the multi-GPU modes and the banded exact path; 11800: mvbev_conv3x3_wino_bf16x3_dgrad (row-Winograd data gradient, output-side mask); 11700: channels-last sources for the fused warps (mvbev_warp_views_wino_rows, mvbev_warp_views_upsampled_wino_rows), mvbev_nchw_to_nhwc_f32; 11600: the non-finite-feature guard (mvbev_warp_views_exact_f32; the fused warps' nonfinite report; gate arguments of mvbev_conv3x3_f32 / mvbev_conv3x3_cout1_f32; mvbev_bev_plan.guard); 11500: row-Winograd conv2 -> conv3 partials (mvbev_wino_rows_split_bf16_dil, mvbev_conv3x3_wino_bf16x3_dil, mvbev_conv3x3_wino_bf16x3_cout1_partials); 11400: mvbev_warp_nonfinite_views (non-finite geometry routes to the direct conv1); the NMS candidate order replays torch's CPU sort (ties included), mvbev_point_nms (no workspace) retired; mvbev_conv3x3_bf16x3_sched / _sched3 retired (forward schedules measured slower); 11300: row-Winograd conv1 (mvbev_pack_conv3x3_weight_wino, mvbev_wino_rows_split_bf16, mvbev_conv3x3_wino_bf16x3); 11200: mvbev_conv3x3_bf16x3_sched3 (schedules over the edge-strip tiles); 11100: edge-strip conv tiles (mvbev_conv_ring_tile_space, mvbev_conv3x3_bf16x3_ex3); 11000: ring-kernel schedules (mvbev_conv_schedule, mvbev_conv3x3_bf16x3_sched, mvbev_conv3x3_dgrad_bf16x3_sched); 10900: mvbev_conv3x3_wgrad_bf16x3_ex2 (pre-split dy rows), mvbev_split_rows_bf16; 10800: mvbev_warp_upsampled_adjoint_plan (training from backbone features), mvbev_conv3x3_cout1_backward_ex; 10700: training on split-bf16 y1 (mvbev_relu_backward_split_f32, mvbev_conv3x3_dgrad_bf16x3_ex); 10600: conv2 -> conv3 fused (mvbev_conv3x3_bf16x3_cout1_partials, mvbev_cout1_reduce_partials); 10500: mvbev_point_nms_ws (any K); 10400: MVBEV_WARP_DST_ZEROED warps; 10300: LDS-DMA ring conv (12-row tiles for split-bf16 input); 10200: native backward (10100: frustum masks, split-K tail, fused upsample+warp) */

/* Bilinear homography warp, zero padding, align_corners=True (kornia 0.6.11).
 *   src    : [B][C][H][W] fp32, element strides src_strides[4] (any, >= 0)
 *   m      : device fp32 [B][3][3] row-major src_norm <- dst_norm (kornia's
 *            _torch_inverse_cast(normalize_homography(M, (H,W), (Ho,Wo))))
 *   dst    : [B][C][Ho][Wo] fp32 at element strides dst_strides[4]
 *            (dst_strides[3] must be 1); may point into a larger tensor. */
int mvbev_warp_perspective_f32(const float* src, int64_t B, int64_t C, int64_t H, int64_t W,
                               const int64_t src_strides[4], const float* m,
                               float* dst, int64_t Ho, int64_t Wo, const int64_t dst_strides[4],
                               void* stream);

/* Same with fp16 storage for src and dst (fp32 coordinate and blend math). */
int mvbev_warp_perspective_f16(const void* src, int64_t B, int64_t C, int64_t H, int64_t W,
                               const int64_t src_strides[4], const float* m,
                               void* dst, int64_t Ho, int64_t Wo, const int64_t dst_strides[4],
                               void* stream);

/* One view of a batched warp: all views share B, C, H, W, Ho, Wo. */
typedef struct mvbev_warp_view {
  const void* src;           /* [B][C][H][W] device, element strides src_strides */
  int64_t src_strides[4];
  void* dst;                 /* [B][C][Ho][Wo] device view, element strides dst_strides ([3] == 1) */
  int64_t dst_strides[4];
  float m[9];                /* src_norm <- dst_norm (row-major), same for every batch item */
} mvbev_warp_view;

/* Warp every view of a frame in ONE launch (the detector's per-camera loop at
 * persp_trans_detector.py:62-75, warp + concat).  views: host array of nviews (<= 16). */
int mvbev_warp_views_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C,
                         int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* stream);
/* Same, writing the split-bf16 blocked layout (MVBEV_LAYOUT_SPLIT_BF16) the 3xbf16 conv
 * reads without any conversion: for (batch, group of 8 channels, row, col) 32 bytes = bf16
 * hi[8] then bf16 lo[8], value = hi + lo.  dst_strides are in 32-byte units
 * {batch, channel group, row, col (must be 1)}; channels beyond C in the last group are 0.
 * src is fp32 (src_is_f16 = 0) or fp16.  (ABI 11600: the flag-less form is retired.)
 * flags of the _ex warps.  MVBEV_WARP_DST_ZEROED: the caller guarantees every dst already
 * holds zeros wherever the view's sample falls outside the source (e.g. a persistent slab
 * zero-filled at allocation and only ever written by this warp with the same matrices), so
 * those pixels — exactly 0 in the result — are skipped instead of rewritten.  Pixels with
 * non-finite coordinates (NaN output) are always written. */
#define MVBEV_WARP_DST_ZEROED 1
/* flag of mvbev_warp_views_wino_rows (ABI 11900): the sources are fp16 (fp32 math; T split-bf16 as for
 * fp32 sources) — config 4's fp16 features on the fused warp + B^T and the row-Winograd conv1. */
#define MVBEV_WARP_SRC_F16 2
/* MVBEV_WARP_WINO43 (ABI 12400; mvbev_warp_views_wino_rows_ex / _upsampled_wino_rows_ex): the fused warp
 * writes the F(4,3) transform T43 (mvbev_wino43_rows_bytes' layout) instead of T; r3_rows then counts
 * four-row tiles (4 * ceil(out_rows / 16)), 3 per 14 x 16 block; the block's staging-box table is
 * mvbev_warp_wino_boxes' with r3_rows = 4 * ceil(r4_rows / 3) (the same 12-row blocks). */
#define MVBEV_WARP_WINO43 4
/* MVBEV_WARP_SRC_BF16 (added after 12500; mvbev_version() stays 12500): the channels-last backbone maps of
 * mvbev_warp_views_upsampled_wino_rows / _ex are bf16 — with MVBEV_WARP_SRC_F16, which those two entry points now
 * take too, what a bf16 / fp16 autocast backbone emits.  Only the loads change (a 32-channel group is 64 B): every
 * value converts to fp32 exactly and all arithmetic is the fp32 form's, so T is bit for bit the T of the same maps
 * cast to fp32.  Both bits together, or either with maps that are not channels-last sources, return
 * MVBEV_ERR_SHAPE; mvbev_warp_views_wino_rows / _ex (already-upsampled features) refuse this bit. */
#define MVBEV_WARP_SRC_BF16 8
int mvbev_warp_views_split_bf16_ex(const mvbev_warp_view* views, int nviews, int src_is_f16,
                                   int64_t B, int64_t C, int64_t H, int64_t W, int64_t Ho, int64_t Wo,
                                   int flags, void* stream);
/* Row windows (ABI 11900): view i's dst holds out_rows rows of the Ho-row grid starting at grid row
 * row0s[i] (host int32 array; 0 <= row0s[i], row0s[i] + out_rows <= Ho), so one launch can warp the row
 * windows the multi-GPU band exchange sends (several entries may share a source).  nonfinite (may be
 * NULL): nf_tag is stored into the device int32 *nonfinite when a sample the warp produces is non-finite
 * (a NaN / inf feature it reads, or non-finite coordinates) — the non-finite guard's report, as the
 * fused row-Winograd warps give it. */
int mvbev_warp_views_split_bf16_rows(const mvbev_warp_view* views, const int32_t* row0s, int nviews, int src_is_f16,
                                     int64_t B, int64_t C, int64_t H, int64_t W, int64_t Ho, int64_t Wo,
                                     int64_t out_rows, int flags, int32_t* nonfinite, int32_t nf_tag, void* stream);
/* Gated zero fill: bytes (a multiple of 16, 16-B aligned dst) of zeros when *gate == gate_tag, else no
 * write (ABI 11900: re-zeroes the band exchange's send chunks after a frame whose exact path wrote them). */
int mvbev_zero_gated(void* dst, int64_t bytes, const int32_t* gate, int32_t gate_tag, void* stream);
/* Gated store (ABI 12200): fp32 src [B][C][H][W] (element strides, src_strides[3] == 1) into dst when
 * *gate == gate_tag, else no write.  dst_layout MVBEV_LAYOUT_F32: fp32 at element strides (dst_strides[3]
 * == 1); MVBEV_LAYOUT_SPLIT_BF16: the split-bf16 blocked layout, dst_strides in 32-byte units {batch,
 * channel group, row, col (1)}, a non-finite value stored as hi = value, lo = 0 (hi + lo keeps it; the
 * fast path's split gives lo = NaN).  The training forward's non-finite guard stores its exact-path
 * activations (conv1's input, y1, y2) where the native backward reads them
 * (persp_trans_detector.py:65-81 under trainer.py:38-47). */
int mvbev_store_gated_f32(const float* src, const int64_t src_strides[4], void* dst, const int64_t dst_strides[4],
                          int64_t B, int64_t C, int64_t H, int64_t W, int dst_layout, const int32_t* gate,
                          int32_t gate_tag, void* stream);
/* Fused bilinear upsample + warp.  views[i].src is the
 * backbone-resolution map [B][C][h][w] that persp_trans_detector.py:65 upsamples with
 * F.interpolate(size=(H, W), mode='bilinear', align_corners=False) before the warp at :69;
 * every bilinear corner of the warp is that upsample evaluated on the fly (one 3x3 source
 * window per output pixel), so the [B][C][H][W] intermediate is never written.  m is the
 * kornia matrix for the UPSAMPLED size (H, W) — the same one mvbev_warp_views_* take.
 * Upsampling only (H >= h, W >= w).  out_layout: MVBEV_LAYOUT_F32 (fp32 src) or
 * MVBEV_LAYOUT_SPLIT_BF16 (fp32 or fp16 src); dst strides as in the entry points above.
 * NaN/inf in the source map are outside the contract (a zero-weight tap of the window may
 * propagate them). */
int mvbev_warp_views_upsampled(const mvbev_warp_view* views, int nviews, int src_is_f16,
                               int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                               int64_t Ho, int64_t Wo, int out_layout, void* stream);
int mvbev_warp_views_upsampled_ex(const mvbev_warp_view* views, int nviews, int src_is_f16,
                                  int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                                  int64_t Ho, int64_t Wo, int out_layout, int flags, void* stream);
/* Frustum mask for the conv (see mvbev_conv3x3_bf16x3_ex): for output tiles of tile_h x
 * tile_w pixels over grid rows [row0, row0 + rows) of the Ho x Wo warp output, bit s of
 * mask[tile] is set when view s's warp (views[s].m, src size H x W) can be non-zero
 * anywhere in the tile grown by `halo` pixels — some pixel samples inside the source, or
 * its coordinates are non-finite (NaN output).  Uses the warp kernels' own fp32 coordinate
 * code, so a clear bit is exact.  Only views[].m is read; nviews <= 16. */
int mvbev_warp_tile_mask(const mvbev_warp_view* views, int nviews, int64_t H, int64_t W,
                         int64_t Ho, int64_t Wo, int64_t row0, int64_t rows, int64_t tile_h,
                         int64_t tile_w, int64_t halo, uint32_t* mask, void* stream);
/* *bits (device uint32, overwritten) = the views (bit s = views[s], nviews <= 16) whose warp has
 * an output pixel of the Ho x Wo grid with non-finite sample coordinates, i.e. a NaN in the warped
 * features of persp_trans_detector.py:69 (a degenerate homography; kornia's 0/0 meshgrid when Ho
 * or Wo is 1).  The warp kernels' own fp32 coordinate code.  Only views[].m is read.  The
 * row-Winograd conv1 mixes a 3-row tile's rows before its products, so a caller routes such
 * geometry to the direct conv, which keeps NaN to the taps that read it as the reference's
 * nn.Conv2d (:51) does. */
int mvbev_warp_nonfinite_views(const mvbev_warp_view* views, int nviews, int64_t H, int64_t W, int64_t Ho,
                               int64_t Wo, uint32_t* bits, void* stream);
/* fp16 storage for src and dst, fp32 math. */
int mvbev_warp_views_f16(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C,
                         int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* stream);

/* Coord-map channels: dst[b][0][v][u] = u/(Wo-1)*2-1, dst[b][1][v][u] = v/(Ho-1)*2-1
 * (computed in float64, rounded to fp32 as numpy->torch does at :106-107). */
int mvbev_fill_coord_map_f32(float* dst, int64_t B, int64_t Ho, int64_t Wo,
                             const int64_t dst_strides[4], void* stream);

/* Number of floats of the packed weight buffer for Cout output channels and K packed
 * input channels (K rounded up to MVBEV_CONV_KC). */
size_t mvbev_conv3x3_packed_floats(int64_t Cout, int64_t K);

/* Re-lay an nn.Conv2d weight w[Cout][Cin_w][3][3] (contiguous fp32, device) into the MFMA
 * staging layout for K packed input channels: packed channel k takes weight channel
 * chan_map[k] (device int32[K]; -1 = zero weights), or k itself when chan_map is NULL
 * (then K must equal Cin_w).  Lets the fused tensor's channel order differ from the
 * module's (view-major slots, coord channels handled separately). */
int mvbev_pack_conv3x3_weight_f32(const float* w, int64_t Cout, int64_t Cin_w,
                                  const int32_t* chan_map, int64_t K, float* w_packed,
                                  void* stream);
/* The same pack, run only when *gate == gate_tag (ABI 12200): the training forward's non-finite guard
 * re-packs the exact path's fp32 weights every step (the optimizer changes them) at the cost of a launch
 * that exits at once when the features are finite. */
int mvbev_pack_conv3x3_weight_f32_gated(const float* w, int64_t Cout, int64_t Cin_w, const int32_t* chan_map,
                                        int64_t K, float* w_packed, const int32_t* gate, int32_t gate_tag,
                                        void* stream);

/* Geometry of one conv launch (all sizes in elements). */
typedef struct mvbev_conv_desc {
  int64_t B;             /* batch items */
  int64_t K;             /* packed input channels (multiple of MVBEV_CONV_KC) */
  int64_t H, W;          /* full image (ground grid) height / width */
  int64_t group;         /* channels per contiguous channel group (multiple of KC, divides K) */
  int64_t group_stride;  /* elements between consecutive channel groups */
  int64_t batch_stride;  /* elements between consecutive batch items */
  int64_t in_row0;       /* global row held by input-buffer row 0 */
  int64_t in_rows;       /* rows in the input buffer (channel plane = in_rows * W) */
  int64_t out_row0;      /* first global output row computed */
  int64_t out_rows;      /* output rows computed (y holds exactly these rows) */
} mvbev_conv_desc;

/* y = act(conv3x3(x, w, dilation=d, padding=d) [+ bias] [+ init]), fp32 MFMA, fp32 accumulate.
 *   x      : input channel ci of item b at x + (ci/group)*group_stride + b*batch_stride
 *            + (ci%group)*in_rows*W  ([B][K][H][W]: group=K; view-major [S][B][C][H][W]: group=C)
 *   w_packed : from mvbev_pack_conv3x3_weight_f32 with the same Cout and K
 *   bias   : [Cout] or NULL;  init : [Cout][H][W] (full-size, broadcast over B) or NULL
 *   relu   : 0/1 (NaN-preserving);  dilation : 1 or 2
 *   y      : [B][Cout][out_rows][W] contiguous fp32, Cout % MVBEV_CONV_BN == 0
 *   Zero padding at the image border; input rows outside the buffer are read as zero, so
 *   a band caller must supply every row the output band needs. */
int mvbev_conv3x3_f32(const float* x, const mvbev_conv_desc* desc, const float* w_packed,
                      const float* bias, const float* init, int64_t Cout, int dilation,
                      int relu, float* y, const int32_t* gate, int32_t gate_tag, void* stream);
/* The same with a row-banded output (ABI 11900): y_band_rows > 0 puts global output row g at row
 * g % y_band_rows of band g / y_band_rows of y = [bands][B][Cout][y_band_rows][W] — the partial-sum
 * multi-GPU mode's reduce-scatter input (as mvbev_conv3x3_wino_bf16x3's band_rows); 0 = the plain y. */
int mvbev_conv3x3_f32_ex(const float* x, const mvbev_conv_desc* desc, const float* w_packed, const float* bias,
                         const float* init, int64_t Cout, int dilation, int relu, float* y, int64_t y_band_rows,
                         const int32_t* gate, int32_t gate_tag, void* stream);
/* y = relu?(y + init) in place (NaN-preserving ReLU) for y [B][C][rows][W] holding grid rows
 * [row0, row0 + rows) of init [C][H][W]; stores tag into the device int32 *flag (NULL: no report) when a
 * result is non-finite (ABI 11900: the coord term + bias + ReLU of the partial-sum mode's summed conv1
 * pre-activation — persp_trans_detector.py:51 — and its non-finite guard). */
int mvbev_bias_relu_nonfinite_f32(float* y, const float* init, int64_t B, int64_t C, int64_t rows, int64_t W,
                                  int64_t H, int64_t row0, int relu, int32_t* flag, int32_t tag, void* stream);
/* conv1's coord term (ABI 12300; persp_trans_detector.py:103-112 coord map, :77 its concat, :51 conv1):
 * out [Cout][H][W] fp32 = bias (NULL: 0) + conv2d over the two coord channels [x = col / (W-1) * 2 - 1,
 * y = row / (H-1) * 2 - 1] (float64 then float, zero padding 1) with conv1's weights w1 [Cout][cin][3][3]
 * at input channels coord_c0 (x) and coord_c0 + 1 (y).  The input-independent part of conv1, added as its
 * accumulators' initial value. */
int mvbev_coord_term_f32(const float* w1, int64_t cin, int64_t coord_c0, const float* bias, int64_t Cout, int64_t H,
                         int64_t W, float* out, void* stream);
/* The same with the parameters' non-finite scan riding on it (ABI 12500; nf_word NULL: as above): nf_tag is stored
 * into the device int32 *nf_word when a value of the term is non-finite (a NaN / inf coord weight or bias, or an
 * overflow) or when one of the two small fp32 arrays extra0 [n0], extra1 [n1] (conv2's bias, conv3's weight; may
 * be NULL / 0) holds a NaN / inf — in training, where the weights change every step, the scan costs no launch. */
int mvbev_coord_term_f32_ex(const float* w1, int64_t cin, int64_t coord_c0, const float* bias, int64_t Cout,
                            int64_t H, int64_t W, float* out, int32_t* nf_word, int32_t nf_tag, const float* extra0,
                            int64_t n0, const float* extra1, int64_t n1, void* stream);
/* Non-finite PARAMETERS (ABI 12500; map_classifier's weights after a diverging optimizer.step(),
 * persp_trans_detector.py:51-54 under trainer.py:47-48).  The fast path cannot keep the reference's NaN / inf
 * pattern under them: its frustum mask never multiplies a masked view's w1 columns (the reference computes
 * 0 * NaN = NaN), the hi/lo bf16 split of +-inf is (inf, NaN) and the Winograd weight transform G w takes
 * differences of weights (inf - inf = NaN), where the reference keeps x * -inf = -inf, which ReLU turns into 0.
 * mvbev_params_nonfinite_f32: params / counts are HOST arrays of nparams (1 .. 8) device fp32 arrays and their
 * lengths; tag is stored into the device int32 *word when any value is NaN / inf (a fresh tag per weight
 * version: no reset, no host sync) — once per weight version, beside the packs and the coord term.
 * mvbev_flag_raise: *flag = flag_tag when *word == word_tag (one thread, in stream order) — arms a frame's
 * non-finite guard (the gate of the exact path below) from that word. */
int mvbev_params_nonfinite_f32(const float* const* params, const int64_t* counts, int nparams, int32_t* word,
                               int32_t tag, void* stream);
int mvbev_flag_raise(const int32_t* word, int32_t word_tag, int32_t* flag, int32_t flag_tag, void* stream);
/* gate (this entry point, mvbev_conv3x3_cout1_f32, mvbev_warp_views_exact_f32; ABI 11600): a device
 * int32; when non-NULL the launch does its work only if *gate == gate_tag at the time it runs (every
 * workgroup exits at once otherwise) — a decision taken on the device in stream order, so a caller
 * can enqueue a conditional path without a host sync (the non-finite guard of mvbev_bev_fuse and
 * the Python engine).  NULL: always run. */

/* Input layouts of mvbev_conv3x3_bf16x3 (descriptor strides are always in 4-byte
 * "channel-element" units, i.e. as for an fp32 tensor of the same logical shape). */
#define MVBEV_LAYOUT_F32 0        /* plain fp32 channel planes */
#define MVBEV_LAYOUT_F16 1        /* plain fp16 channel planes (strides in elements) */
#define MVBEV_LAYOUT_SPLIT_BF16 2 /* per (8-channel group, pixel): bf16 hi[8], bf16 lo[8] */
#define MVBEV_LAYOUT_SPLIT_ROWS 3 /* per (channel, row, 8-pixel run): bf16 hi[8], bf16 lo[8]
                                     (W % 8 == 0; the same bytes per row as fp32) */
#define MVBEV_LAYOUT_SPLIT_BF16_PIX 4 /* pixel-major split-bf16: per (pixel, 8-channel group) bf16 hi[8], lo[8],
                                         [B][rows][W][C/8] (ABI 12100): the conv data gradients' output for the
                                         warp adjoint, whose gather then reads a pixel's channels in one piece */

/* 3xbf16 split-precision variant of mvbev_conv3x3_f32 (mvbev_conv3x3_bf16x3_ex below; same
 * descriptor and semantics): a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 MFMA, fp32
 * accumulation; ~2^-16 relative per product (fp32-class; see conv_bf16x3.hip).  x_layout:
 * MVBEV_LAYOUT_* (fp32, the config-4 fp16 slab, or the pre-split slab).
 * Weights packed by mvbev_pack_conv3x3_weight_bf16x3 (bytes: mvbev_conv3x3_packed_bytes_bf16x3). */
size_t mvbev_conv3x3_packed_bytes_bf16x3(int64_t Cout, int64_t K);
int mvbev_pack_conv3x3_weight_bf16x3(const float* w, int64_t Cout, int64_t Cin_w,
                                     const int32_t* chan_map, int64_t K, void* w_packed,
                                     void* stream);
/* Output tile of mvbev_conv3x3_bf16x3_ex (rows x columns), the granule of group_mask below:
 * MVBEV_CONV_TILE_H rows for fp32/fp16 input; split-bf16 input (the LDS-DMA ring kernel)
 * uses the row count mvbev_conv3x3_bf16x3_tile_rows returns (12). */
#define MVBEV_CONV_TILE_H 8
#define MVBEV_CONV_TILE_W 32
int mvbev_conv3x3_bf16x3_tile_rows(int x_layout, int dilation);

/* The 3xbf16 conv (ABI 11600: the form without mask / order / workspace is retired).
 *   y, y_layout: MVBEV_LAYOUT_F32 ([B][Cout][out_rows][W] fp32, as above) or
 *     MVBEV_LAYOUT_SPLIT_BF16 ([B][Cout/8][out_rows][W] pieces of bf16 hi[8], lo[8]: the
 *     next conv's input without a conversion pass).
 *   group_mask (optional, device): one uint32 per output tile, tiles row-major over
 *     ceil(out_rows / tile_rows(x_layout, dilation)) x ceil(W / MVBEV_CONV_TILE_W) (rows from out_row0);
 *     bit g clear = input channel group g (desc->group channels, group % 16 == 0, at most 32
 *     groups) is exactly zero over the tile and its 3x3 dilated halo, so its K-chunks are
 *     skipped for that tile (identical result).  mvbev_warp_tile_mask builds it from the
 *     views' homographies: a camera's warped features are exactly 0 outside its frustum.
 *   tile_order (optional, device, with group_mask): the B x tiles pixel tiles (index
 *     (b * tiles_y + tile_y) * tiles_x + tile_x) in the order to run them — heaviest
 *     first evens out the per-tile work the mask makes uneven.
 *   workspace (optional, device): scratch for the split-K tail — when the output tiles do
 *     not fill a whole number of rounds over the CUs (one workgroup per CU), the tiles of
 *     the last, partial round are cut into K-ranges run by separate workgroups and a second
 *     launch sums each tile's pieces in K order (deterministic).  workspace_bytes() returns
 *     what this shape needs (0 = not used); a NULL / smaller workspace keeps whole tiles.
 *     Not combined with group_mask. */
size_t mvbev_conv3x3_bf16x3_workspace_bytes(const mvbev_conv_desc* desc, int64_t Cout);
int mvbev_conv3x3_bf16x3_ex(const void* x, int x_layout, const mvbev_conv_desc* desc,
                            const void* w_packed, const float* bias, const float* init,
                            int64_t Cout, int dilation, int relu, void* y, int y_layout,
                            const uint32_t* group_mask, const int32_t* tile_order, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Pixel-tile spaces of the split-bf16-input (ring) conv.  MVBEV_TILES_GRID: the 12 x 32 tile
 * grid of mvbev_conv3x3_bf16x3_ex (tiles_y x ceil(W / 32) per batch item, row-major; the last
 * tile column computes up to 31 columns past W).  MVBEV_TILES_EDGE_STRIP (0 < W % 32 <= 16):
 * the 12 x 32 grid over columns [0, 32 * floor(W / 32)), then edge_tiles tiles of edge_rows x EW
 * pixels (EW = 8 or 16, edge_rows = 384 / EW) over the last W % 32 columns, top to bottom — the
 * same 384 pixels per tile and no MFMA column past W (Wildtrack's W = 360: 11 regular tile
 * columns + 3 strips of 48 x 8).  mvbev_conv_ring_tile_space fills
 * g = {tiles_x, tiles_y, edge_tiles, EW, edge_rows} for desc's output rows and W (0 edges for
 * the grid), or returns MVBEV_ERR_SHAPE when the space does not apply. */
#define MVBEV_TILES_GRID 0
#define MVBEV_TILES_EDGE_STRIP 1
int mvbev_conv_ring_tile_space(const mvbev_conv_desc* desc, int tile_space, int64_t g[5]);
/* mvbev_conv3x3_bf16x3_ex with the tiles of tile_space (split-bf16 x only, no workspace):
 * group_mask[pp] / tile_order (b * tiles + pp) index pixel tiles pp of that space (edge-strip
 * masks: mvbev_warp_tile_mask with tile_h = edge_rows, tile_w = EW, last tile column).
 * MVBEV_TILES_EDGE_STRIP: dilation 1 with ReLU (conv1, map_classifier[0:2]).  Same y, bitwise,
 * as the grid tiles. */
int mvbev_conv3x3_bf16x3_ex3(const void* x, int x_layout, const mvbev_conv_desc* desc,
                             const void* w_packed, const float* bias, const float* init,
                             int64_t Cout, int dilation, int relu, void* y, int y_layout,
                             const uint32_t* group_mask, const int32_t* tile_order, int tile_space,
                             void* stream);

/* Row-Winograd form of the forward conv1 (map_classifier[0:2], persp_trans_detector.py:51-52,
 * dilation 1): F(3,3) along the rows, y = A^T [(G w) . (B^T d)] per kernel column, 5 instead of 9
 * MFMA K-blocks per (16-channel chunk, kernel column); same 3xbf16 split products, fp32 accumulate.
 * Replaces the same call as mvbev_conv3x3_bf16x3_ex with dilation 1 (the reference's
 * nn.Conv2d(512*N+2, 512, 3, padding=1) forward, :51), in two steps:
 *   1. mvbev_wino_rows_split_bf16: the split-bf16 input x (desc as mvbev_conv3x3_bf16x3_ex) ->
 *      T = B^T over each 3-row output tile's 5 input rows, split-bf16 blocked
 *      [B][K/8][5 * 4 * ceil(out_rows / 12)][hi, lo][W][8] (mvbev_wino_rows_bytes; ABI 11500: a row's hi plane, then
 *      its lo plane — was [W][hi, lo][8]).  With
 *      group_mask (12 x 32 tiles, as the conv) the cleared (tile, group) pairs are not written:
 *      T must then be zero-filled once and only ever written by this call with the same mask.
 *   2. mvbev_conv3x3_wino_bf16x3: y from T (desc: B, K, H, W, group, out_row0, out_rows as in
 *      step 1), weights from mvbev_pack_conv3x3_weight_wino (same arguments as
 *      mvbev_pack_conv3x3_weight_bf16x3), bias / init / relu / y / y_layout / group_mask /
 *      tile_order as mvbev_conv3x3_bf16x3_ex (grid tiles, 12 x 32). */
/* Warp + the row transform of step 1 in one pass, from fp32 sources (mvbev_warp_views_split_bf16's
 * views and matrices): the T rows of r3_rows 3-row output tiles (3 * r3_rows >= Ho; the conv's
 * T has 4 * ceil(out_rows / 12) of them) are written for each view's channels at its dst, whose
 * dst_strides are in 32-byte units: [0] per batch item, [1] per 8-channel group, [2] per T row
 * (= Wo: the row's hi plane, then its lo plane), [3] = 1 — the view's slice of T.  The warped slab itself is never written.  flags:
 * MVBEV_WARP_DST_ZEROED = T is zero-filled and only written by this geometry, so a (tile,
 * column) whose 5 samples all fall outside the source is skipped.  Replaces :69 + :77 + the
 * first step of conv1 (:51) for inference. */
int mvbev_warp_views_wino_rows(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t H,
                               int64_t W, int64_t Ho, int64_t Wo, int64_t r3_rows, int flags, int32_t* nonfinite,
                               int32_t nf_tag, void* stream);
/* (ABI 12200) The per-(view, block) source boxes of the NCHW form of mvbev_warp_views_wino_rows, once per
 * geometry (views[i].m only; src / dst unused): boxes = device int32 [nviews][mvbev_warp_wino_boxes_count(Wo,
 * r3_rows)][4], 16-B aligned.  Passed to mvbev_warp_views_wino_rows_ex (same views, sizes and r3_rows), every
 * block of a (view, tile) takes its staging box from the table instead of reducing it, and a block none of
 * whose samples falls inside the source (with MVBEV_WARP_DST_ZEROED) returns at once; boxes = NULL is
 * mvbev_warp_views_wino_rows.  Channels-last sources (the line-per-pixel kernel, same block tiles) use it for the
 * early return only. */
int64_t mvbev_warp_wino_boxes_count(int64_t Wo, int64_t r3_rows);
int mvbev_warp_wino_boxes(const mvbev_warp_view* views, int nviews, int64_t H, int64_t W, int64_t Ho, int64_t Wo,
                          int64_t r3_rows, int32_t* boxes, void* stream);
int mvbev_warp_views_wino_rows_ex(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t H,
                                  int64_t W, int64_t Ho, int64_t Wo, int64_t r3_rows, int flags, int32_t* nonfinite,
                                  int32_t nf_tag, const int32_t* boxes, void* stream);
/* The same from backbone-resolution maps [B][C][h][w] (fp32, unit column stride, w >= 4): the
 * fused 3x upsample + warp of mvbev_warp_views_upsampled (m for the upsampled size H x W) and the
 * row transform in one pass (the detector's inference path, :65 + :69 + :77 + conv1's first step).
 * ABI 11700, both fused warps: channels-last sources (src_strides[1] == 1, [3] >= C, the other strides
 * multiples of 4 floats, 16-B aligned, C % 32 == 0; the same logical [B][C][h][w] tensor in torch's
 * channels_last memory format) run a line-per-pixel form (one 128-B line holds a pixel's 32 channels
 * of a block); same T up to fp32 rounding of the bilinear sums.
 * Added after 12500 (mvbev_version() stays 12500): with MVBEV_WARP_SRC_F16 or MVBEV_WARP_SRC_BF16 in flags the
 * channels-last maps are fp16 / bf16 (src_strides[1] == 1, [3] >= C, the other strides multiples of 8 elements,
 * 16-B aligned, C % 32 == 0): the same T, bit for bit, as from those maps cast to fp32. */
int mvbev_warp_views_upsampled_wino_rows(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t h,
                                         int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int64_t r3_rows,
                                         int flags, int32_t* nonfinite, int32_t nf_tag, void* stream);
/* (ABI 12200) As mvbev_warp_wino_boxes for the channels-last upsample warp: the per-(view, block) boxes of the
 * blocks' 3x3 backbone windows (h x w maps, m for the upsampled H x W), once per geometry; passed to
 * mvbev_warp_views_upsampled_wino_rows_ex (same views, sizes and r3_rows) every block of a (view, tile) takes its
 * staging box from the table and a block none of whose samples falls inside the source (with
 * MVBEV_WARP_DST_ZEROED) returns at once.  The table has mvbev_warp_wino_boxes_count(Wo, r3_rows) entries per
 * view; NCHW maps ignore it. */
int mvbev_warp_upsampled_wino_boxes(const mvbev_warp_view* views, int nviews, int64_t h, int64_t w, int64_t H,
                                    int64_t W, int64_t Ho, int64_t Wo, int64_t r3_rows, int32_t* boxes, void* stream);
int mvbev_warp_views_upsampled_wino_rows_ex(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t h,
                                            int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int64_t r3_rows,
                                            int flags, int32_t* nonfinite, int32_t nf_tag, const int32_t* boxes,
                                            void* stream);
/* nonfinite (both fused warps, ABI 11600; NULL = no report): nf_tag is stored into the device int32
 * *nonfinite when a sample reads a NaN / inf feature (conservatively also when finite values overflow).
 * The fused form folds B^T (and the upsample's taps into one 3x3 window), so it cannot keep the
 * reference's NaN / inf pattern for such features; the caller's exact path, gated on the report, can:
 *   mvbev_warp_views_exact_f32 — the warp (h = H, w = W) or the 3x upsample + warp (h x w backbone
 *   maps, persp_trans_detector.py:65 + :69) in the reference's own evaluation order: per in-bounds
 *   corner the PyTorch upsample value (both taps of each axis multiplied, zero weights included; no
 *   fma contraction in the source index), times its grid_sample weight; out-of-bounds corners selected
 *   to 0.  fp32 src [B][C][h][w], fp32 dst [B][C][Ho][Wo] at element strides ([3] == 1); gate as
 *   mvbev_conv3x3_f32's. */
int mvbev_warp_views_exact_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t h, int64_t w,
                               int64_t H, int64_t W, int64_t Ho, int64_t Wo, const int32_t* gate, int32_t gate_tag,
                               void* stream);
/* The same on row windows and fp16 sources (ABI 11900): view i's dst holds out_rows rows of the Ho-row
 * grid starting at grid row row0s[i] (host int32 array) — the exact path in row bands of bounded memory,
 * and the band exchange's windows; src_kind: 0 = fp32 sources, 1 = fp16, 2 = bf16 (added after 12500, the
 * argument was src_is_f16: 0 and 1 mean what they meant; fp32 math), anything else MVBEV_ERR_SHAPE. */
int mvbev_warp_views_exact_rows(const mvbev_warp_view* views, const int32_t* row0s, int nviews, int src_kind,
                                int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int64_t Ho,
                                int64_t Wo, int64_t out_rows, const int32_t* gate, int32_t gate_tag, void* stream);
/* NCHW -> channels-last copy (ABI 11700): view i's fp32 [B][C][H][W] map at views[i].src /
 * src_strides into a contiguous [B][H][W][C] buffer at views[i].dst (dst_strides, m ignored), every
 * view in one launch — the input of the channels-last fused upsample warp for NCHW producers. */
int mvbev_nchw_to_nhwc_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C, int64_t H, int64_t W,
                           void* stream);
/* The same for elements of elem_size bytes (added after 12500; mvbev_version() stays 12500): 4 (as above) or 2 —
 * fp16 / bf16 maps, a plain transposition of their bits; strides in elements; anything else MVBEV_ERR_SHAPE. */
int mvbev_nchw_to_nhwc_ex(const mvbev_warp_view* views, int nviews, int elem_size, int64_t B, int64_t C, int64_t H,
                          int64_t W, void* stream);
size_t mvbev_conv3x3_packed_bytes_wino(int64_t Cout, int64_t K);
int mvbev_pack_conv3x3_weight_wino(const float* w, int64_t Cout, int64_t Cin_w, const int32_t* chan_map,
                                   int64_t K, void* w_packed, void* stream);
/* The same with the parameters' non-finite scan riding on it (ABI 12500; nf_word NULL: as above): nf_tag is
 * stored into the device int32 *nf_word when a weight the pack reads (every tap of every mapped input channel)
 * is NaN / inf. */
int mvbev_pack_conv3x3_weight_wino_ex(const float* w, int64_t Cout, int64_t Cin_w, const int32_t* chan_map,
                                      int64_t K, void* w_packed, int32_t* nf_word, int32_t nf_tag, void* stream);
size_t mvbev_wino_rows_bytes(const mvbev_conv_desc* desc);
int mvbev_wino_rows_split_bf16(const void* x, const mvbev_conv_desc* desc, const uint32_t* group_mask, void* t,
                               size_t t_bytes, void* stream);
int mvbev_conv3x3_wino_bf16x3(const void* t, const mvbev_conv_desc* desc, const void* w_packed, const float* bias,
                              const float* init, int64_t Cout, int relu, void* y, int y_layout, int64_t y_band_rows,
                              const uint32_t* group_mask, const int32_t* tile_order, void* stream);
/* y_band_rows (ABI 11600; MVBEV_LAYOUT_F32 only, 0 = plain [B][Cout][out_rows][W]): y in row bands,
 * computed row r (from out_row0) at band r / y_band_rows, y = [bands][B][Cout][y_band_rows][W] (rows
 * past out_rows in the last band untouched) — the reduce-scatter input of the partial-sum multi-GPU
 * mode, written in place. */
/* The same two steps for dilation 2 (conv2, map_classifier[2:4], persp_trans_detector.py:53:
 * nn.Conv2d(512, 512, 3, padding=2, dilation=2)): the 12-row workgroup tile holds two interleaved
 * pairs of 3-row tiles (rows r, r + 2, r + 4), whose T = B^T over the 5 input rows r - 2 ... r + 6
 * (step 2); a kernel column's taps are 2 columns apart.  mvbev_wino_rows_split_bf16_dil(dilation 1)
 * is mvbev_wino_rows_split_bf16; T has the same size (mvbev_wino_rows_bytes).  The conv: no init,
 * no mask (dense), y fp32 or split-bf16 (_dil), or, replacing
 * mvbev_conv3x3_bf16x3_cout1_partials (same desc, bias, w3, partials layout and size; relu,
 * dilation 2), conv3's partial sums from the epilogue (_cout1_partials, ABI 11500). */
int mvbev_wino_rows_split_bf16_dil(const void* x, const mvbev_conv_desc* desc, int dilation,
                                   const uint32_t* group_mask, void* t, size_t t_bytes, void* stream);
/* The same transform, run only when *gate == gate_tag (gate not NULL; ABI 12200): the training guard's
 * T / T2 of its exact-path conv1 input / y1 for the native weight gradients. */
int mvbev_wino_rows_split_bf16_gated(const void* x, const mvbev_conv_desc* desc, int dilation,
                                     const uint32_t* group_mask, void* t, size_t t_bytes, const int32_t* gate,
                                     int32_t gate_tag, void* stream);
int mvbev_conv3x3_wino_bf16x3_dil(const void* t, const mvbev_conv_desc* desc, const void* w_packed, const float* bias,
                                  int64_t Cout, int dilation, int relu, void* y, int y_layout, void* stream);
int mvbev_conv3x3_wino_bf16x3_cout1_partials(const void* t, const mvbev_conv_desc* desc, const void* w_packed,
                                             const float* bias, int64_t Cout, int dilation, int relu, const float* w3,
                                             void* partials, size_t partials_bytes, void* stream);
/* Row-Winograd F(4,3) (ABI 12400; persp_trans_detector.py:51 conv1 and :53-54 conv2 -> conv3): the same
 * convs as mvbev_conv3x3_wino_bf16x3 / _cout1_partials from 6 transformed rows per 4 output rows (points
 * 0, +-1, +-2, inf) instead of 5 per 3 — 10 % fewer MFMAs, the K sum walked xi-major.  T43 =
 * [B][K/8][6 * 4 * ceil(out_rows / 16)][hi, lo][W][8] (mvbev_wino43_rows_bytes; dilation 2: row tile q of
 * a 16-row tile holds rows 8 (q / 2) + q % 2 + 2 pt), written by mvbev_wino43_rows_split_bf16 from the
 * split-bf16 input; weights from mvbev_pack_conv3x3_weight_wino43 (arguments as
 * mvbev_pack_conv3x3_weight_wino); group_mask / tile_order over 16 x 32 output tiles
 * (mvbev_warp_tile_mask with 16-row tiles); y fp32 or split-bf16. */
size_t mvbev_conv3x3_packed_bytes_wino43(int64_t Cout, int64_t K);
int mvbev_pack_conv3x3_weight_wino43(const float* w, int64_t Cout, int64_t Cin_w, const int32_t* chan_map, int64_t K,
                                     void* w_packed, void* stream);
size_t mvbev_wino43_rows_bytes(const mvbev_conv_desc* desc);
int mvbev_wino43_rows_split_bf16(const void* x, const mvbev_conv_desc* desc, int dilation, const uint32_t* group_mask,
                                 void* t, size_t t_bytes, void* stream);
int mvbev_conv3x3_wino43_bf16x3(const void* t, const mvbev_conv_desc* desc, const void* w_packed, const float* bias,
                                const float* init, int64_t Cout, int dilation, int relu, void* y, int y_layout,
                                const uint32_t* group_mask, const int32_t* tile_order, void* stream);
int mvbev_conv3x3_wino43_bf16x3_cout1_partials(const void* t, const mvbev_conv_desc* desc, const void* w_packed,
                                               const float* bias, int64_t Cout, int dilation, int relu,
                                               const float* w3, void* partials, size_t partials_bytes, void* stream);
/* A data gradient as the dilation-1 row-Winograd conv (ABI 11800; the training backward's conv1
 * dgrad, persp_trans_detector.py:51 differentiated): t = the row transform of the split-bf16 dy
 * (mvbev_wino_rows_split_bf16), w_packed = mvbev_pack_conv3x3_weight_wino of the weight with its
 * in / out channels swapped and its taps reversed ([Cout = forward Cin][forward Cout][3][3]), no
 * bias / init / ReLU; dx fp32 or split-bf16 [B][Cout][out_rows][W].  out_mask (optional, int32 per
 * 12 x 32 output tile as mvbev_warp_tile_mask): tiles of output channel group g (cot_per_group
 * 128-channel tiles) whose bit g is clear are not written (a consumer that never reads them). */
/* The data-gradient weights of mvbev_conv3x3_wino_bf16x3_dgrad straight from the forward weight
 * w [Cout_f][Cin_f][3][3] fp32 (ABI 11800): packed as mvbev_pack_conv3x3_weight_wino would pack
 * w'[o][i][kh][kw] = w[i][o][2 - kh][2 - kw] for o < Cout (Cout % 128 == 0, Cout <= Cin_f: the
 * first Cout forward input channels) and i < Cout_f (the packed K). */
int mvbev_pack_conv3x3_weight_wino_dgrad(const float* w, int64_t Cout_f, int64_t Cin_f, int64_t Cout, void* w_packed,
                                         void* stream);
int mvbev_conv3x3_wino_bf16x3_dgrad(const void* t, const mvbev_conv_desc* desc, const void* w_packed, int64_t Cout,
                                    void* dx, int dx_layout, const uint32_t* out_mask, int64_t cot_per_group,
                                    void* stream);

/* conv2 -> conv3 without conv2's activation in HBM (map_classifier[2:5],
 * persp_trans_detector.py:53-54, inference): the split-bf16-input conv of
 * mvbev_conv3x3_bf16x3_ex (desc, w_packed, bias, Cout, dilation, relu as there; no init, no
 * mask) whose epilogue, instead of storing y, writes per (Cout tile, 64-channel half) set s,
 * tap t of the following single-output conv and computed pixel the partial
 *   partials[b][s][t][row - desc->out_row0][col] = sum over the set's channels co of
 *                                                  w3[co][t] * act(y[b][co][row][col])
 * (w3 : [Cout][3][3] fp32, the next conv's weight; 2 * Cout / MVBEV_CONV_BN sets;
 * partials_bytes >= mvbev_conv3x3_bf16x3_cout1_partials_bytes).  mvbev_cout1_reduce_partials
 * then forms map[b][0][r][:] = conv3x3(y, w3, dilation3, padding dilation3)[map_row0 + r]
 * summing the sets' shifted taps in a fixed order; the rows map_row0 +- dilation3 that lie
 * inside the image must be among desc's computed rows.  Same value as storing y and running
 * mvbev_conv3x3_cout1_f32 on it, to fp32 summation order. */
size_t mvbev_conv3x3_bf16x3_cout1_partials_bytes(const mvbev_conv_desc* desc, int64_t Cout);
int mvbev_conv3x3_bf16x3_cout1_partials(const void* x, const mvbev_conv_desc* desc, const void* w_packed,
                                        const float* bias, int64_t Cout, int dilation, int relu, const float* w3,
                                        void* partials, size_t partials_bytes, void* stream);
int mvbev_cout1_reduce_partials(const void* partials, const mvbev_conv_desc* desc, int64_t Cout, int dilation3,
                                float* map, int64_t map_row0, int64_t map_rows, void* stream);
/* The same with mvbev_flag_raise folded in (ABI 12500; word NULL: as above): *flag = flag_tag when *word ==
 * word_tag, stored by the launch's first thread — inference's per-frame raise of the non-finite guard from the
 * parameters' word costs no launch of its own (the gated exact path is enqueued behind this kernel). */
int mvbev_cout1_reduce_partials_ex(const void* partials, const mvbev_conv_desc* desc, int64_t Cout, int dilation3,
                                   float* map, int64_t map_row0, int64_t map_rows, const int32_t* word,
                                   int32_t word_tag, int32_t* flag, int32_t flag_tag, void* stream);

/* y[b][0][r][:] = conv3x3(x[b], w, dilation=d, padding=d)[out_row0 + r], one output channel,
 * no bias.  x : [B][C][in_rows][W] holding global rows [in_row0, in_row0+in_rows) of an
 * H x W image;  w : [C][3][3] contiguous fp32;  y : [B][1][out_rows][W]. */
int mvbev_conv3x3_cout1_f32(const float* x, int64_t B, int64_t C, int64_t H, int64_t W,
                            int64_t in_row0, int64_t in_rows, int64_t out_row0, int64_t out_rows,
                            const float* w, int dilation, float* y, const int32_t* gate, int32_t gate_tag,
                            void* stream);
/* The same with flags (ABI 12500).  MVBEV_COUT1_SAME_SIZE_INTERP: persp_trans_detector.py:82's F.interpolate of
 * the map to its own size applied to every output value — the identity on finite values and NaN, but torch's
 * lerp x + 0 * (x' - x) turns +-inf into NaN at that pixel.  The fast path elides that call (its map is finite);
 * the non-finite guard's exact path, whose conv3 can give an inf under a non-finite w3 or y2, sets the flag so
 * that its map keeps the reference's pattern.  Another bit: MVBEV_ERR_SHAPE.  word (NULL: none): mvbev_flag_raise
 * folded in, as in mvbev_cout1_reduce_partials_ex — the training forward's conv3 arms the step's guard. */
#define MVBEV_COUT1_SAME_SIZE_INTERP 1
int mvbev_conv3x3_cout1_f32_ex(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, int64_t in_row0,
                               int64_t in_rows, int64_t out_row0, int64_t out_rows, const float* w, int dilation,
                               float* y, int flags, const int32_t* gate, int32_t gate_tag, const int32_t* word,
                               int32_t word_tag, int32_t* flag, int32_t flag_tag, void* stream);

/* ---- one-call project + fuse ----------------------------------------------
 * The inference hot path of PerspTransDetector.forward after the backbone
 * (persp_trans_detector.py:62-82: the per-view warp at :69 (+ the 3x upsample of :65 for
 * backbone-resolution sources), the concat at :77, map_classifier at :81, the identity
 * interpolate at :82) for a caller that does not want to orchestrate the entry points above
 * itself.  Three calls over one caller-owned device workspace:
 *   mvbev_bev_plan_init      host only: validates the geometry, lays out the workspace
 *   mvbev_bev_fuse_prepare   once per geometry and weight version: conv1's packing (G w for the
 *                            row-Winograd form), conv2's, the coord term (conv1 bias + conv1 over
 *                            the 2 coord channels, :21), the frustum mask, the heavy-first tile
 *                            order and the non-finite-geometry check; ONE stream sync (the mask
 *                            and the check are read back to plan the launches)
 *   mvbev_bev_fuse           per frame, enqueued, no sync: map = [B][1][Ho][Wo] fp32
 * Weights are the nn.Conv2d parameters of map_classifier (:51-54), fp32 contiguous device
 * tensors: w1 [512][N*C+2][3][3], b1 [512], w2 [512][512][3][3], b2 [512], w3 [1][512][3][3];
 * b2 and w3 are read again by every mvbev_bev_fuse (keep them alive and unchanged; after an
 * update of any weight call prepare again).  The module's channel order is view-major (view v's
 * channels are v*C .. v*C + C-1, then the 2 coord channels) as torch.cat builds it at :77. */
#define MVBEV_BEV_MAX_VIEWS 16
#define MVBEV_BEV_SRC_F32 0          /* views[v]: [B][C][H][W] fp32 contiguous (kornia's input, :69) */
#define MVBEV_BEV_SRC_F16 1          /* views[v]: [B][C][H][W] fp16 contiguous (fp32 math) */
#define MVBEV_BEV_SRC_BACKBONE_F32 2 /* views[v]: [B][C][h][w] fp32 backbone maps; :65's upsample fused */
#define MVBEV_BEV_SRC_CHANNELS_LAST 16 /* flag OR'ed into an fp32 kind (ABI 11700): views[v] hold the same
                                          tensor channels-last, [B][H][W][C] ([B][h][w][C]) contiguous, C % 32
                                          == 0 — the fused warps' line-per-pixel kernels */
#define MVBEV_BEV_NO_GUARD 32        /* flag (ABI 11900): no non-finite guard — no guard regions in the
                                        workspace (the guard's fp32 slab is one row chunk of at most 1 GiB) */
typedef struct mvbev_bev_geometry {
  int32_t num_views;                /* N, 1 .. 16 (persp_trans_detector.py:58-59) */
  int32_t src_kind;                 /* MVBEV_BEV_SRC_* */
  int64_t B, C;                     /* batch items; channels per view */
  int64_t h, w;                     /* backbone map size (MVBEV_BEV_SRC_BACKBONE_F32 only) */
  int64_t H, W;                     /* the warp's source size (upsample_shape, :23) */
  int64_t Ho, Wo;                   /* the ground grid (reducedgrid_shape) */
  float m[MVBEV_BEV_MAX_VIEWS][9];  /* per view: kornia's src_norm <- dst_norm of proj_mats[v] (:68-69) */
} mvbev_bev_geometry;
typedef struct mvbev_bev_plan {     /* host memory, caller-owned; filled by the calls below */
  mvbev_bev_geometry g;
  int32_t wino;                     /* after prepare: 1 = row-Winograd conv1, 0 = direct (non-finite geometry);
                                       ABI 12400: 2 = row-Winograd F(4,3) (grids whose rows fill 16-row tiles) */
  int32_t frustum;                  /* conv1 skips the views a tile's camera frustum excludes (C % 16 == 0 after padding) */
  int32_t prepared;
  int32_t wino2;                    /* after prepare: 1 = row-Winograd conv2 -> conv3 partials (ABI 11500; finite geometry);
                                       ABI 12400: 2 = F(4,3) (16-row tiles and a launch >= 8 rounds deep) */
  int32_t guard;                    /* 1 = the non-finite-feature guard runs behind the row-Winograd path (ABI 11600) */
  int64_t Cs, tiles;                /* channels per view slot (C rounded to 8); conv1's 12 x 32 tiles (16 x 32 with wino 2) */
  size_t off[24];                   /* workspace regions */
  size_t workspace_bytes;           /* >= what mvbev_bev_fuse_workspace_bytes returns, 256-B aligned base */
  const float* b2;
  const float* w3;
  int32_t params_nonfinite;         /* after prepare (ABI 12500): 1 = w1 / b1 / w2 / b2 / w3 hold a NaN / inf, so
                                       every frame takes the guard's exact path (guard plans only) */
} mvbev_bev_plan;
int mvbev_bev_plan_init(const mvbev_bev_geometry* g, mvbev_bev_plan* plan);
size_t mvbev_bev_fuse_workspace_bytes(const mvbev_bev_geometry* g);
int mvbev_bev_fuse_prepare(mvbev_bev_plan* plan, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, void* workspace, size_t ws_bytes, void* stream);
/* views: host array of N device pointers (layout per src_kind); map: [B][1][Ho][Wo] fp32.  fp32
 * sources: the warp writes conv1's row-Winograd transform directly; fp16 sources (and geometry
 * with non-finite samples) run the direct conv1 on the split slab.  guard (fp32 sources, ABI
 * 11600): the warp reports a NaN / inf feature it samples into a device flag, and the exact path
 * (mvbev_warp_views_exact_rows into an fp32 slab window, mvbev_conv3x3_f32 twice, mvbev_conv3x3_cout1_f32,
 * each gated on that flag) rewrites the map with the reference's NaN / inf pattern — decided on the
 * device, no host sync; launches that exit at once when the features are finite.  ABI 11900: in
 * output-row chunks whose fp32 slab window holds at most 1 GiB (one chunk at configs 1, 2 and 4);
 * MVBEV_BEV_NO_GUARD in src_kind turns the guard and its workspace regions off.  ABI 12500: prepare (which
 * reads the weights and synchronises already) also looks for a NaN / inf in w1, b1, w2, b2, w3
 * (mvbev_params_nonfinite_f32) and keeps the answer in plan->params_nonfinite; a guard plan then starts every
 * frame with the flag set, so the exact path writes the map (no extra launch: the flag's per-frame reset stores
 * the tag instead of 0).  b2 and w3 are read per frame: a caller that changes them in place prepares again. */
int mvbev_bev_fuse(const mvbev_bev_plan* plan, const void* const* views, float* map, void* workspace,
                   size_t ws_bytes, void* stream);

/* ---- native backward: training through the hot path ----------------
 * Replaces the autograd of the stock ops the reference trains through (trainer.py:38-49,
 * loss.backward() at :47): grid_sample's backward under kornia.warp_perspective
 * (persp_trans_detector.py:69) and nn.Conv2d / nn.ReLU backward of map_classifier (:51-54). */

/* Adjoint of mvbev_warp_views_* (bilinear, zeros padding, align_corners=True): for every output
 * pixel whose sample point is finite and inside, each in-bounds corner of the source gradient
 * gets w_corner * grad_out (fp32 atomic adds; no gradient from zero-padded or NaN samples).
 *   views[i].src : grad_out, [B][C][Ho][Wo] fp32 at element strides src_strides
 *   views[i].dst : grad_src, [B][C][H][W] fp32 at element strides dst_strides ([3] must be 1);
 *                  ACCUMULATED into (zero it first for a plain gradient)
 *   views[i].m   : the forward's src_norm <- dst_norm matrix. */
int mvbev_warp_views_backward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t C,
                                  int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* stream);

/* The same adjoint as a deterministic gather (no atomics in the per-channel loop).
 * mvbev_warp_adjoint_plan builds, once per view geometry (m = src_norm <- dst_norm, host
 * array), the CSR transpose of the warp's sparse sampling matrix: for source pixel p, entries
 * row_ptr[p] .. row_ptr[p+1]-1 hold (col = output pixel v*Wo+u, val = bilinear corner weight)
 * in increasing col order.  Device buffers: row_ptr int32[H*W + 1], col int32[4*Ho*Wo], val
 * fp32[4*Ho*Wo] (capacity; row_ptr[H*W] = entries used), scratch int32[H*W]. */
int mvbev_warp_adjoint_plan(const float* m, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int32_t* row_ptr,
                            int32_t* col, float* val, int32_t* scratch, void* stream);
/* The same plan for the fused 3x-upsample + warp of mvbev_warp_views_upsampled (the backbone
 * map h x w upsampled to H x W, persp_trans_detector.py:65, then warped, :69): source pixels are
 * the h x w backbone pixels, <= 9 entries per output pixel (the sample's 3x3 backbone window,
 * weight = upsample weight x warp weight, zero-weight cells omitted).  Buffers: row_ptr
 * int32[h*w + 1], col int32[9*Ho*Wo], val fp32[9*Ho*Wo], scratch int32[h*w].  With it,
 * mvbev_warp_views_adjoint (H, W = h, w) takes the gradient straight to the backbone features. */
int mvbev_warp_upsampled_adjoint_plan(const float* m, int64_t h, int64_t w, int64_t H, int64_t W, int64_t Ho,
                                      int64_t Wo, int32_t* row_ptr, int32_t* col, float* val, int32_t* scratch,
                                      void* stream);

typedef struct mvbev_warp_adjoint_view {
  const float* grad_out;       /* [B][C][Ho][Wo] fp32, element strides (row / column dense) */
  int64_t grad_out_strides[4];
  float* grad_src;             /* [B][C][H][W] fp32, element strides (row / column dense) */
  int64_t grad_src_strides[4];
  const int32_t* row_ptr;      /* the view's plan */
  const int32_t* col;
  const float* val;
} mvbev_warp_adjoint_view;

/* grad_src (accumulate ? += : =) S^T grad_out for every view, one launch (nviews <= 16).
 * grad_out_layout MVBEV_LAYOUT_F32 (element strides) or MVBEV_LAYOUT_SPLIT_BF16 (grad_out =
 * the view's first 8-channel group of a split-bf16 blocked tensor, 16-B aligned, strides in
 * 32-byte units {batch, channel group, row = Wo, col = 1}; value = hi + lo), or (ABI 12100)
 * MVBEV_LAYOUT_SPLIT_BF16_PIX (the same pieces pixel-major: strides {batch, 1, Wo * G, G} with
 * G >= C / 8 groups per pixel; C % 8 == 0) — same grad_src values as the split layout. */
int mvbev_warp_views_adjoint(const mvbev_warp_adjoint_view* views, int nviews, int grad_out_layout, int64_t B,
                             int64_t C, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int accumulate,
                             void* stream);

/* A host-built schedule for the LDS-DMA ring kernel (split-bf16 input, dilation 1 or 2): block i
 * runs items[i] = {tile, c0, c1, slot} — tile = ((b * tiles_y + ty) * tiles_x + tx) * n_cot + cot
 * (12-row tiles, mvbev_conv3x3_bf16x3_tile_rows), chunks [c0, c1) of the tile's active 16-channel
 * chunk sequence (all of K, or the groups a group_mask enables, in order), slot = -1 for a
 * whole tile or the partial-sum slot of a piece of a split tile; tile < 0 = an idle block.
 * fixups[f] = {tile, first slot, pieces, 0}: after the conv, one block per split tile adds its
 * pieces' partial sums in slot order (deterministic) and writes the tile as the kernel would.
 * The order of items is the dispatch order (block i goes to XCD i % 8); the host plans it to
 * balance the CUs (mvdet_amd/schedule.py: e.g. splitting the last, partial round's tiles). */
typedef struct mvbev_conv_schedule {
  const int32_t* items;    /* device [nitems][4], 16-B aligned */
  int32_t nitems;
  const int32_t* fixups;   /* device [nfix][4], 16-B aligned */
  int32_t nfix;
  int32_t nslots;          /* partial slots the items use: 0 .. nslots - 1 */
  void* partials;          /* device, >= nslots * mvbev_conv_schedule_slot_bytes() */
  size_t partial_bytes;
} mvbev_conv_schedule;
size_t mvbev_conv_schedule_slot_bytes(void);
/* mvbev_conv3x3_dgrad_bf16x3_ex (split-bf16 dy only) run as scheduled (the training backward's
 * conv1 data gradient; out_mask as there). */
int mvbev_conv3x3_dgrad_bf16x3_sched(const void* dy, int dy_layout, const mvbev_conv_desc* desc,
                                     const void* w_packed, int64_t Cout_p, int dilation, void* dx, int dx_layout,
                                     const uint32_t* out_mask, int64_t cot_per_group,
                                     const mvbev_conv_schedule* sched, void* stream);

/* Weights for the data gradient of a 3x3 stride-1 conv with padding = dilation: that gradient is
 * the same conv over dy with w'[k][co][t] = w[co][k][8 - t], so mvbev_conv3x3_bf16x3_ex computes
 * it with these weights (Cout' = round_up(K_out, MVBEV_CONV_BN) output channels, K' = Cout_w).
 * Output channel o of the dgrad conv is forward input channel chan_map[o] (device int32[K_out],
 * -1 = zero; NULL = identity).  w: forward weight [Cout_w][Cin_w][3][3] fp32.  Size:
 * mvbev_conv3x3_packed_bytes_bf16x3(round_up(K_out, 128), Cout_w). */
int mvbev_pack_conv3x3_dgrad_bf16x3(const float* w, int64_t Cout_w, int64_t Cin_w,
                                    const int32_t* chan_map, int64_t K_out, void* w_packed,
                                    void* stream);
/* The same pack, run only when *gate == gate_tag (gate NULL: always; ABI 12500), and a gated tile
 * mask, dst[i] = src[i] when *gate == gate_tag else 0 (n uint32 words): the training backward's non-finite
 * guard.  conv1's row-Winograd data gradient mixes the dy1 rows under a 3-row tile before the products, so a
 * NaN / inf of dy1 (a non-finite w2) would spread over its tile; behind it the direct data gradient
 * (mvbev_conv3x3_dgrad_bf16x3_ex with these gated weights and the gated frustum mask as out_mask) rewrites the
 * tiles when the forward's flag fired, and every workgroup of it leaves at once (an all-zero mask) when not. */
int mvbev_pack_conv3x3_dgrad_bf16x3_gated(const float* w, int64_t Cout_w, int64_t Cin_w, const int32_t* chan_map,
                                          int64_t K_out, void* w_packed, const int32_t* gate, int32_t gate_tag,
                                          void* stream);
int mvbev_mask_gated_u32(const uint32_t* src, int64_t n, uint32_t* dst, const int32_t* gate, int32_t gate_tag,
                         void* stream);

/* The data-gradient conv itself: mvbev_conv3x3_bf16x3_ex over dy (fp32, desc as for a forward
 * conv over [B][Cout_w][H][W]) with the dgrad packing, no bias / ReLU, dx in dx_layout
 * (MVBEV_LAYOUT_F32 or MVBEV_LAYOUT_SPLIT_BF16), plus an output-side mask: with out_mask
 * (device, one uint32 per output tile as group_mask of the _ex form), the tiles of output
 * channel group g (cot_per_group consecutive 128-channel Cout tiles, e.g. one camera's
 * channels) are skipped where bit g is clear — those dx entries are left unwritten, for a
 * consumer that never reads them (the warp adjoint reads a view's gradient only where the
 * view samples inside its source, which the frustum mask of mvbev_warp_tile_mask bounds). */
/* dy in dy_layout: MVBEV_LAYOUT_F32 or MVBEV_LAYOUT_SPLIT_BF16 (the LDS-DMA ring kernel, dilation 1
 * or 2; its output tiles, and so out_mask's tiles, are mvbev_conv3x3_bf16x3_tile_rows(
 * MVBEV_LAYOUT_SPLIT_BF16, dilation) rows high). */
int mvbev_conv3x3_dgrad_bf16x3_ex(const void* dy, int dy_layout, const mvbev_conv_desc* desc, const void* w_packed,
                                  int64_t Cout_p, int dilation, void* dx, int dx_layout, const uint32_t* out_mask,
                                  int64_t cot_per_group, void* stream);

/* Weight gradient of mvbev_conv3x3_bf16x3_ex (3xbf16 MFMA, fp32 accumulation):
 *   dw[co][chan_map[k]][t] = sum_b,y,x dy[b][co][y][x] * x[b][k][y + (t/3-1)d][x + (t%3-1)d]
 * x as in the forward (desc: whole image, in_row0 = out_row0 = 0, in_rows = out_rows = H;
 * x_layout MVBEV_LAYOUT_F32 or MVBEV_LAYOUT_SPLIT_BF16); dy [B][Cout][H][W] fp32 contiguous,
 * Cout % 128 == 0; dw [Cout][Cin_w][3][3] fp32 — only the channels chan_map names are written
 * (chan_map NULL = identity, K <= Cin_w).  dilation 1 or 2.  workspace: device scratch of
 * mvbev_conv3x3_wgrad_workspace_bytes() (per-partition partial sums; the reduction over
 * partitions runs in a fixed order, so the result is deterministic). */
size_t mvbev_conv3x3_wgrad_workspace_bytes(const mvbev_conv_desc* desc, int64_t Cout);
/* Optional chunk lists (both NULL = every chunk): skip the pixel chunks where an input-channel
 * group (desc->group channels, a multiple of 64: one camera's slot of the fused slab) is exactly
 * zero over the 3x3 window: chunk_list[chunk_off[g] .. chunk_off[g+1]) lists, ascending, the chunks
 * (row segments of 32 pixels, index (b * H + y) * ceil(W / 32) + x / 32) where group g can be
 * non-zero (from the frustum mask of mvbev_warp_tile_mask with halo >= dilation).  Device int32.
 * dy in dy_layout: MVBEV_LAYOUT_F32 or MVBEV_LAYOUT_SPLIT_ROWS (dy pre-split by
 * mvbev_split_rows_bf16; the LDS-DMA wgrad path only: split-bf16 x, dilation 1 or 2, W % 8 == 0,
 * else MVBEV_ERR_SHAPE) — bitwise the same dw as from the fp32 dy (the kernel splits an fp32 dy
 * with the same rounding), without the per-segment split pass.  (ABI 11600: the forms without
 * chunk lists / dy layout are retired.) */
int mvbev_conv3x3_wgrad_bf16x3_ex2(const void* x, int x_layout, const mvbev_conv_desc* desc,
                                   const void* dy, int dy_layout, int64_t Cout, int dilation,
                                   const int32_t* chan_map, int64_t Cin_w, float* dw,
                                   const int32_t* chunk_list, const int32_t* chunk_off, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* Row-Winograd weight gradient of a 3x3 conv of dilation 1 or 2 (ABI 12000; conv1 / conv2 of
 * map_classifier, persp_trans_detector.py:51, 53, whose forward ran mvbev_conv3x3_wino_bf16x3[_dil]).  With
 * the forward's y = A^T[(G w) . (B^T d)] per 3-row tile r3 (conv_bf16x3.hip), dW[co][ci][kh][kw] =
 * sum_xi G[xi][kh] M_xi[kw] where
 *   M_xi[kw][co][ci] = sum_{b, r3, x} D_xi[co][r3][x] T_xi[ci][r3][x + dil (kw - 1)],
 *   D_xi = sum_j AT[j][xi] dy[base(r3) + dil j]  (base: the forward's row tiles — 3 r3, or conv2's interleaved ones):
 * t is the forward's transform (mvbev_wino_rows_split_bf16[_dil] / the fused warp's T, t_bytes of it),
 * dy_wino is D (mvbev_wino_dy_rows_f32 of the same dilation), and the products run 3xbf16 as in
 * mvbev_conv3x3_wgrad_bf16x3_ex2, whose arguments the others mean (chunk lists: chunk (b * R3 + r3) *
 * ceil(W / 32) + x / 32 where T_xi of group g can be non-zero — the forward's 12-row frustum mask, tile
 * r3 / 4; R3 = ceil(H / 3) for dilation 1, 4 ceil(H / 12) for dilation 2).  x0.556 of the direct form's
 * MFMAs; W % 8 == 0, desc over all rows, 128-channel groups with chunk lists.  workspace:
 * mvbev_conv3x3_wgrad_wino_workspace_bytes. */
size_t mvbev_wino_dy_rows_bytes(int64_t B, int64_t Cout, int64_t H, int64_t W, int dilation);
/* D[b][xi][co][r3] (r3 < R3, rows past H zero) of fp32 dy [B][Cout][H][W] in MVBEV_LAYOUT_SPLIT_ROWS;
 * AT = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 1]; W % 8 == 0, 16-B aligned. */
int mvbev_wino_dy_rows_f32(const float* dy, int64_t B, int64_t Cout, int64_t H, int64_t W, int dilation,
                           void* out, size_t out_bytes, void* stream);
size_t mvbev_conv3x3_wgrad_wino_workspace_bytes(const mvbev_conv_desc* desc, int64_t Cout, int dilation);
int mvbev_conv3x3_wgrad_wino_bf16x3(const void* t, size_t t_bytes, const mvbev_conv_desc* desc, const void* dy_wino,
                                    size_t dy_wino_bytes, int64_t Cout, int dilation, const int32_t* chan_map,
                                    int64_t Cin_w, float* dw, const int32_t* chunk_list, const int32_t* chunk_off,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* fp32 rows x [rows][W] (16-B aligned, W % 8 == 0) -> out [rows][W / 8] pieces of bf16 hi[8],
 * lo[8] (MVBEV_LAYOUT_SPLIT_ROWS; hi = bf16(x) round-to-nearest-even, lo = bf16(x - hi)). */
int mvbev_split_rows_bf16(const float* x, int64_t rows, int64_t W, void* out, void* stream);

/* db[co] = sum_b,p dy[b][co][p] (db may be NULL) and, when dw != NULL, the weight gradient of the
 * two coord channels (create_coord_map, persp_trans_detector.py:103-112) that are input channels
 * coord_ch, coord_ch + 1 of a conv of the given dilation: dw[co][coord_ch + j][t] (dw is
 * [Cout][Cin_w][3][3]).  dy [B][Cout][H][W] fp32. */
int mvbev_conv3x3_bias_coord_grad_f32(const float* dy, int64_t B, int64_t Cout, int64_t H, int64_t W,
                                      int dilation, float* db, float* dw, int64_t Cin_w,
                                      int64_t coord_ch, void* stream);

/* In place: dy[i] = y[i] <= 0 ? 0 : dy[i] (y = the ReLU's output; torch threshold_backward: the gradient
 * passes where y is NaN). */
int mvbev_relu_backward_f32(float* dy, const float* y, int64_t n, void* stream);
/* Same (NaN rule included) with y in the split-bf16 layout (y = hi + lo; [B][C/8][H][W] pieces, C % 8 == 0) and
 * dy fp32 [B][C][H][W]; dy_split (optional, 16-B aligned) also receives the masked dy in the
 * split layout (the next data-gradient conv's input). */
int mvbev_relu_backward_split_f32(float* dy, const void* y_split, int64_t B, int64_t C, int64_t H, int64_t W,
                                  void* dy_split, void* stream);

/* Backward of mvbev_conv3x3_cout1_f32 over a whole image (x [B][C][H][W], w [C][3][3], dmap
 * [B][1][H][W] fp32):  dx[b][c][p] = sum_t w[c][t] dmap[b][p - s_t], zeroed where x <= 0 when
 * relu_mask (x is the previous ReLU's output: its backward fused, torch threshold_backward, so dx passes
 * where x is NaN); dw[c][t] = sum_b,p
 * dmap[b][p] x[b][c][p + s_t].  Any output may be NULL; dx_split (C % 8 == 0, 16-B aligned): dx
 * also in the split-bf16 layout ([B][C/8][H][W] pieces of bf16 hi[8], lo[8]), the input of the
 * next data-gradient conv. */
int mvbev_conv3x3_cout1_backward_ex(const float* x, const float* w, const float* dmap, int64_t B, int64_t C,
                                    int64_t H, int64_t W, int dilation, int relu_mask, float* dx, void* dx_split,
                                    float* dw, void* stream);

/* ---- evaluation post-processing (trainer.py:97-106, 148-157) ---- */

/* map > thres over an H x W map, in row-major (torch.nonzero) order: *count = number of hits
 * (device int32), ij[2k], ij[2k+1] = row, column and scores[k] = value of the first
 * min(count, capacity) hits.  One workgroup; enqueued, no host sync. */
int mvbev_threshold_points(const float* map, int64_t H, int64_t W, float thres, int32_t* count,
                           int32_t* ij, float* scores, int64_t capacity, void* stream);

/* Greedy point NMS of multiview_detector/utils/nms.py:7-43 for any K (trainer.py:154 passes every
 * map cell over cls_thres, up to Ho*Wo): the candidates in the order torch's CPU scores.sort(0)
 * produces (nms.py:22; libstdc++ std::sort of (score, index) pairs, NaN largest — replayed
 * exactly, so equal scores come out as on the reference's CPU, not in index order), read from
 * the end, the top_k largest considered; keep the best, drop every later candidate whose
 * distance sqrt(dx^2+dy^2) (fp32, correctly rounded) is not > dist_thres, repeat (nms.py:29-42).
 * points [K][2] fp32, scores [K] fp32 (device); keep [K] int64 = kept indices then zeros;
 * *count (device int32) = number kept.  workspace: device, >= mvbev_point_nms_workspace_bytes,
 * 4-B aligned.  One workgroup; enqueued, no host sync. */
size_t mvbev_point_nms_workspace_bytes(int64_t K, int64_t top_k);
int mvbev_point_nms_ws(const float* points, const float* scores, int64_t K, float dist_thres,
                       int64_t top_k, int64_t* keep, int32_t* count, void* workspace, size_t ws_bytes,
                       void* stream);

/* ---- training criterion (multiview_detector/loss/gaussian_mse.py:7-20, trainer.py:43-56) ----
 * Added after 12400 (mvbev_version() stays 12400): mvbev_adaptive_max_pool_f32,
 * mvbev_gaussian_mse_blocks, mvbev_gaussian_mse_f32, mvbev_loss_finalize_f32,
 * mvbev_gaussian_mse_backward_f32.  All fp32, on the caller's stream, caller-owned buffers, no host
 * sync.  One launch covers a host array of n (<= 16) items; an item is one (prediction, target)
 * pair of mse_loss(x, conv2d(adaptive_max_pool2d(target, x.shape[2:]), kernel, padding=(k-1)/2)). */
typedef struct mvbev_loss_item {
  const float* x;        /* prediction [B][C][h][w], element strides x_strides (any, >= 0); NULL:
                          * only the transformed target is wanted (diff must be NULL too) */
  int64_t x_strides[4];
  const float* target;   /* ground truth [B][C][Ht][Wt], element strides t_strides (any, >= 0) */
  int64_t t_strides[4];
  int64_t C, h, w, Ht, Wt;
  float* pooled;         /* [B][C][h][w] contiguous scratch; unused (may be NULL) when Ht == h && Wt == w */
  float* t_out;          /* optional: the transformed target, [B][C][h][w] contiguous */
  float* diff;           /* optional: x - t, [B][C][h][w] contiguous, kept for the backward */
  int32_t kernel_id;     /* index into the kernels array of mvbev_gaussian_mse_f32 */
  float weight;          /* this item's factor in the total loss (1, or alpha / N) */
} mvbev_loss_item;

/* One uploaded [C][C][k][k] kernel and its host-side plan (made once per kernel version). */
typedef struct mvbev_loss_kernel {
  const float* w;        /* device, contiguous [C][C][k][k] */
  int64_t C, k;          /* C <= 8, k odd */
  uint64_t slice_mask;   /* bit co * C + ci set: slice (co, ci) holds a non-zero (or non-finite) value */
  int32_t finite;        /* every value is finite: the two exact skips (all-zero slice, all-zero
                          * staged target) apply; 0: every tap is multiplied with every target cell
                          * inside the image, so 0 * NaN reaches t (the padding is never multiplied,
                          * as in torch's conv2d) */
} mvbev_loss_kernel;

/* F.adaptive_max_pool2d(target, (h, w)) into pooled for every item whose sizes differ (the others
 * are skipped): window rows floor(i Ht / h) .. ceil((i + 1) Ht / h), columns alike; NaN wins. */
int mvbev_adaptive_max_pool_f32(const mvbev_loss_item* items, int n, int64_t B, void* stream);

/* Workgroups of mvbev_gaussian_mse_f32 over these items = rows of its partials (0: invalid). */
int64_t mvbev_gaussian_mse_blocks(const mvbev_loss_item* items, int n, int64_t B);

/* Per 16 x 64 output tile: the (pooled) target tile plus its (k-1)/2 halo staged into LDS (zeros
 * outside the image), the direct C x C x k x k convolution, d = x - t, t_out / diff when asked,
 * and one row of partials per workgroup: partials[4 g] = sum d^2, [4 g + 1] = #(x > cls_thres and
 * gt == 1), [4 g + 2] = #(x > cls_thres), [4 g + 3] = sum gt — the last three only for item
 * stats_item (-1: none; its target must have x's size), 0 elsewhere.  partials: device fp64,
 * >= 4 * mvbev_gaussian_mse_blocks values.  MVBEV_ERR_SHAPE: even k, C > 8, a kernel whose C
 * differs from the item's, or a tile C (15 + k) (63 + k) floats that does not fit 64 KiB of LDS.
 * No atomics on floats: bitwise repeatable. */
int mvbev_gaussian_mse_f32(const mvbev_loss_item* items, int n, int64_t B, const mvbev_loss_kernel* kernels,
                           int nkernels, float cls_thres, int stats_item, double* partials, int64_t npartials,
                           void* stream);

/* Point-list targets.  Added after 12400 (mvbev_version() stays): mvbev_loss_points,
 * mvbev_gaussian_mse_points_f32.  A record parallel to items[i] that holds the non-zero cells of
 * the item's logical [B][C][Ht][Wt] target instead of the dense tensor: the item's target and pooled
 * are then unused (may be NULL) and no pooling launch is needed for it.  All three pointers NULL: a
 * dense item, handled as by mvbev_gaussian_mse_f32. */
typedef struct mvbev_loss_points {
  const int32_t* cells;    /* device [n][3]: channel, row, column of each cell, every (b, c, row, col) at most
                            * once, sorted by batch item; 0 <= channel < C, 0 <= row < Ht, 0 <= column < Wt */
  const float* values;     /* device [n]: the cells' values, finite and >= 0 (ground truth is counts) */
  const int32_t* offsets;  /* device [B + 1]: batch item b owns cells offsets[b] .. offsets[b + 1] - 1 */
  int64_t Ht, Wt;          /* must equal items[i].Ht, items[i].Wt */
} mvbev_loss_points;

/* mvbev_gaussian_mse_f32 with a record per item (points: host array of n).  For a point item the
 * workgroup zero-fills its LDS tile and raises, for every cell (c, r, q, value) of its batch item, the
 * pooled cells rows floor(r h / Ht) .. ceil((r + 1) h / Ht) - 1, columns floor(q w / Wt) ..
 * ceil((q + 1) w / Wt) - 1 (those whose adaptive_max_pool2d window holds the cell), clipped to the tile
 * plus halo, to the value with an integer maximum: the staged tile, and so every output, is bitwise
 * what mvbev_adaptive_max_pool_f32 + mvbev_gaussian_mse_f32 give on the dense tensor of the same cells.
 * The cell lists are the caller's contract (they live on the device and are not read here); a channel
 * out of range or a value <= 0 is skipped by the kernel, a row or column out of range is clipped.
 * Same return codes as mvbev_gaussian_mse_f32, plus MVBEV_ERR_NULL for points == NULL or a record
 * with some but not all of its pointers, and MVBEV_ERR_SHAPE for a record whose Ht, Wt are not the
 * item's (or exceed 2^31 - 1).  mvbev_gaussian_mse_blocks, the partials, finalize and the backward
 * serve both kinds of item unchanged. */
int mvbev_gaussian_mse_points_f32(const mvbev_loss_item* items, const mvbev_loss_points* points, int n,
                                  int64_t B, const mvbev_loss_kernel* kernels, int nkernels, float cls_thres,
                                  int stats_item, double* partials, int64_t npartials, void* stream);

/* Sums the partials in a fixed order in fp64: *loss = sum_i weight_i sse_i / (B C_i h_i w_i)
 * (fp32); stats (optional, fp64[3]) = tp, fp = pred - tp, fn = gt_sum - tp of item stats_item. */
int mvbev_loss_finalize_f32(const mvbev_loss_item* items, int n, int64_t B, const double* partials,
                            int64_t npartials, int stats_item, float* loss, double* stats, void* stream);

/* grads[i] ([B][C][h][w] contiguous) = *grad_out * weight_i * 2 / numel_i * items[i].diff;
 * grad_out is a device scalar (no sync).  grads: host array of n device pointers. */
int mvbev_gaussian_mse_backward_f32(const mvbev_loss_item* items, int n, int64_t B, const float* grad_out,
                                    float* const* grads, void* stream);

/* ---- image head (persp_trans_detector.py:65-66 after the head's first 1x1 conv) ----
 * Added after 12400 (mvbev_version() stays 12400): mvbev_img_head_forward_f32,
 * mvbev_img_head_backward_blocks, mvbev_img_head_backward_f32, mvbev_img_head_grad_weight_f32.
 *   out = conv2d(relu(F.interpolate(g, (Hu, Wu), mode="bilinear")), weight)    (1x1, no bias)
 * for every view in one launch, fp32.  Per output pixel: the four align_corners=False taps of
 * every channel (all four always multiplied, so 0 * inf and 0 * NaN give NaN as in the reference),
 * ReLU that keeps NaN, then the Co dot products.  The upsampled tensor is never written; the
 * backward recomputes it from g.  Range: Cm <= 256, Co <= 4, Hu >= h, Wu >= w, n <= 16 views, every
 * tensor below 2^31 elements (else MVBEV_ERR_SHAPE; a size <= 0 is MVBEV_ERR_RANK, a negative
 * stride MVBEV_ERR_STRIDE, a missing pointer MVBEV_ERR_NULL). */
typedef struct mvbev_img_head_item {
  const float* g;              /* [B][Cm][h][w], element strides g_strides (any, >= 0): NCHW planes
                                * and torch channels_last both run without a copy */
  int64_t g_strides[4];
  float* out;                  /* forward: [B][Co][Hu][Wu], element strides out_strides */
  int64_t out_strides[4];
  const float* grad_out;       /* backward: d loss / d out, [B][Co][Hu][Wu], strides grad_out_strides;
                                * NULL: this view took no part in the loss (no grad_g is written and it
                                * adds nothing to grad_W) */
  int64_t grad_out_strides[4];
  float* grad_g;               /* backward: [B][Cm][h][w], strides grad_g_strides; NULL: not wanted */
  int64_t grad_g_strides[4];
} mvbev_img_head_item;

/* weight: device [Co][Cm] contiguous.  One workgroup per (view, b, 8 x 32 output tile). */
int mvbev_img_head_forward_f32(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h, int64_t w,
                               int64_t Co, int64_t Hu, int64_t Wu, const float* weight, void* stream);

/* Workgroups of mvbev_img_head_backward_f32 over these items (the views with a grad_out) = columns
 * of its partials (0: invalid arguments or no such view). */
int64_t mvbev_img_head_backward_blocks(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h,
                                       int64_t w, int64_t Co, int64_t Hu, int64_t Wu);

/* grad_g = U^T(mask * (W^T grad_out)) in gather form (every backbone pixel sums the output pixels
 * whose taps reach it, in a fixed order; mask = !(pre <= 0), so the gradient passes at NaN as in
 * threshold_backward), and, when partials is not NULL, the per-workgroup sums of
 * grad_out[o] * relu(pre[c]) as partials[Co * Cm][blocks] (device fp32, npartials >= Co * Cm *
 * mvbev_img_head_backward_blocks values, every one written).  No float atomics: bitwise repeatable. */
int mvbev_img_head_backward_f32(const mvbev_img_head_item* items, int n, int64_t B, int64_t Cm, int64_t h, int64_t w,
                                int64_t Co, int64_t Hu, int64_t Wu, const float* weight, float* partials,
                                int64_t npartials, void* stream);

/* grad_w[Co][Cm] = the row sums of partials[Co * Cm][nblocks], in a fixed order in fp64. */
int mvbev_img_head_grad_weight_f32(const float* partials, int64_t nblocks, int64_t Cm, int64_t Co, float* grad_w,
                                   void* stream);

/* ---- warp-sum head (no_joint_conv_variant.py:64-81 after map_classifier[0] moved in front) ----
 * Added after 12400 (mvbev_version() stays 12400): mvbev_warp_sum_head_forward_f32,
 * mvbev_warp_sum_head_backward_blocks, mvbev_warp_sum_head_backward_f32,
 * mvbev_warp_sum_head_grad_params_f32.
 * The "no joint spatial reasoning" ablation upsamples every view's 512-channel map (:64), warps it
 * (:68), concatenates the views with the two coord channels (:76) and applies Conv2d(512 N + 2, 512, 1),
 * ReLU, Conv2d(512, 1, 1, bias=False) (:51-53, :80).  The 1x1 conv commutes with the upsample and the
 * warp (both linear per channel), so with z_v = W_v feat_v at backbone resolution (a GEMM, the caller's):
 *   hidden[b, :, p] = relu(bias + w_coord . coord(p) + sum_v warp_v(upsample(z_v))[b, :, p])
 *   map[b, 0, p]    = w2 . hidden[b, :, p]
 * in one launch: no upsampled map, no concatenated slab and, with hidden == NULL, nothing of
 * [B][Cm][Ho][Wo] is written.
 *
 * views[i]: src = z_i [B][Cm][h][w] fp32 with channel stride 1 (channels-last lines; batch, row and
 * column strides free, >= 0), m = the kornia matrix for the upsampled size H x W (as
 * mvbev_warp_views_upsampled), dst unused.  bias [Cm], w_coord [Cm][2] (x, y), w2 [Cm], map
 * [B][1][Ho][Wo] contiguous, hidden [B][Cm][Ho][Wo] contiguous planes (the post-ReLU values) or NULL.
 * boxes: NULL, or the int32 [nviews][tiles][4] of mvbev_warp_upsampled_wino_boxes for the same
 * matrices and sizes with r3_rows = 4 ceil(Ho / 12) (geometry only: a view whose box says that it
 * reaches no pixel of a tile is not evaluated there).  The sample window is the folded 3x3 backbone
 * window of mvbev_warp_views_upsampled, the one mvbev_warp_upsampled_adjoint_plan transposes; the
 * coord values are those of mvbev_fill_coord_map_f32.  A pixel whose sample coordinates are not
 * finite for some view is NaN; a pixel outside a view's source gets exactly 0 from that view (its
 * data is not read).  NaN / Inf in z are outside the contract: the commuted order cannot reproduce
 * where the reference's 0 * NaN lands.  NaN / Inf in bias, w_coord and w2 with finite z are inside it
 * (ABI 12500): every product is formed, and an infinite map value is stored as NaN, as :81's
 * F.interpolate of the map to its own size makes it (the identity otherwise).
 * Range: 1 <= nviews <= 16, 1 <= Cm <= 512 (any, not only multiples of 4), H >= h, W >= w (else
 * MVBEV_ERR_SHAPE; a size <= 0 is MVBEV_ERR_RANK, a channel stride != 1 or a negative stride
 * MVBEV_ERR_STRIDE, a missing pointer MVBEV_ERR_NULL). */
int mvbev_warp_sum_head_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t Cm, int64_t h,
                                    int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, const float* bias,
                                    const float* w_coord, const float* w2, float* map, float* hidden,
                                    const int32_t* boxes, void* stream);

/* Columns of mvbev_warp_sum_head_backward_f32's partials: B * ceil(Ho * Wo / 4096) (0: invalid sizes). */
int64_t mvbev_warp_sum_head_backward_blocks(int64_t B, int64_t Cm, int64_t Ho, int64_t Wo);

/* dhidden[b, c, p] = hidden[b, c, p] <= 0 ? 0 : dmap[b, p] * w2[c] (mvbev_relu_backward_f32's rule: the
 * gradient passes where hidden is NaN), [B][Cm][Ho][Wo] planes that may alias hidden (NULL: not
 * wanted), and, when partials is not NULL, the per-workgroup sums partials[4][Cm][blocks] (blocks =
 * mvbev_warp_sum_head_backward_blocks) of dmap * hidden (grad_w2), dhidden (grad_bias), dhidden * x and
 * dhidden * y (grad_w_coord), every one written.  The gradient to z_v is mvbev_warp_views_adjoint of
 * dhidden with the plan of mvbev_warp_upsampled_adjoint_plan.  No float atomics: bitwise repeatable. */
int mvbev_warp_sum_head_backward_f32(const float* dmap, const float* hidden, const float* w2, int64_t B, int64_t Cm,
                                     int64_t Ho, int64_t Wo, float* dhidden, float* partials, void* stream);

/* grad_w2 [Cm], grad_bias [Cm], grad_w_coord [Cm][2] (each may be NULL: not wanted) = the row sums of
 * partials[4 * Cm][nblocks], in a fixed order in fp64. */
int mvbev_warp_sum_head_grad_params_f32(const float* partials, int64_t nblocks, int64_t Cm, float* grad_w2,
                                        float* grad_bias, float* grad_w_coord, void* stream);

/* ---- thin fused conv1 (res_proj_variant.py:53, :70-82: the "late fusion" head's first conv) ----
 * Added after 12400 (mvbev_version() stays 12400): mvbev_thin_conv1_forward_f32,
 * mvbev_thin_conv1_backward_blocks, mvbev_thin_conv1_backward_f32, mvbev_thin_conv1_grad_weight_f32.
 * The late-fusion ablation warps ONE plane per view (the foot channel of the image result, :72), concatenates
 * the N warped planes with the two coord channels (:81) and applies Conv2d(N + 2, Cout, 3, padding=1), ReLU
 * (:53).  In one launch:
 *   x[b][c][r][u], c < N      = the kornia warp of view c's plane (mvbev_warp_perspective_f32's coordinates,
 *                               bilinear blend and zero padding; non-finite coordinates give NaN)
 *   x[b][N], x[b][N + 1]      = the coord values of mvbev_fill_coord_map_f32
 *   y1[b][co][r][u]           = relu(b1[co] + sum_{c < N + 2} sum_{kh, kw} w1[co][c][kh][kw] x[b][c][r + kh - 1][u + kw - 1])
 * with x zero outside the grid (coord channels included: nn.Conv2d's padding), products and sums in fp32 in a
 * fixed order, a ReLU that keeps NaN, and every tap multiplied: a NaN sample reaches exactly its 3 x 3
 * neighbourhood in every output channel.  A view whose samples over a tile and its halo all fall outside its
 * source adds exact zeros and is not evaluated there (geometry only).
 *
 * views[i]: src = the plane [B][1][H][W] fp32 at element strides src_strides (batch and row strides >= 0, column
 * stride 1, the channel stride is not read: a channel slice of a wider tensor runs without a copy), m = the
 * kornia matrix; dst unused.  w1 [Cout][N + 2][3][3] fp32 contiguous (the module's own tensor, no packing),
 * b1 [Cout] or NULL.  y1 contiguous in y1_layout: MVBEV_LAYOUT_F32 ([B][Cout][Ho][Wo]) or
 * MVBEV_LAYOUT_SPLIT_BF16 ([B][Cout / 8][Ho][Wo] pieces of bf16 hi[8], lo[8], 16-B aligned: the input of
 * mvbev_wino_rows_split_bf16_dil and the ring conv).  xw (NULL in inference): the N warped planes,
 * [B][N][Ho][Wo] fp32 contiguous, which the backward reads.  NaN / Inf in the planes are outside the contract
 * (a view skipped over a tile does not multiply them).  NaN / Inf in the weights (ABI 12500) are inside it
 * through mvbev_thin_conv1_forward_f32_ex: w_mask (NULL: as this entry point) is a device int32 whose bit v says
 * that view v's columns w1[:, v] hold a non-finite value (mvbev_thin_conv1_weight_mask, once per weight
 * version); such a view is evaluated over every tile, so its zero samples meet the weight (0 * NaN = NaN, the
 * reference's pixels).  With finite weights the word is 0 and y1 is bitwise this entry point's.
 * Range: 1 <= nviews <= 16, Cout % 8 == 0, every tensor below 2^31 elements (else MVBEV_ERR_SHAPE, as an
 * unknown layout; a size <= 0 is MVBEV_ERR_RANK, a column stride != 1 or a negative stride MVBEV_ERR_STRIDE, a
 * missing pointer MVBEV_ERR_NULL, a misaligned split y1 MVBEV_ERR_ALIGN). */
int mvbev_thin_conv1_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W, int64_t Ho,
                                 int64_t Wo, const float* w1, const float* b1, int64_t Cout, void* y1, int y1_layout,
                                 float* xw, void* stream);
int mvbev_thin_conv1_forward_f32_ex(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W,
                                    int64_t Ho, int64_t Wo, const float* w1, const float* b1, int64_t Cout, void* y1,
                                    int y1_layout, float* xw, const int32_t* w_mask, void* stream);
/* *mask (device int32) = bit v set when w1[:, v] (v < nviews of the [Cout][nviews + 2][3][3] weight) holds a
 * NaN / inf; one workgroup, every launch writes the whole word (no reset needed). */
int mvbev_thin_conv1_weight_mask(const float* w1, int nviews, int64_t Cout, int32_t* mask, void* stream);

/* Workgroups of mvbev_thin_conv1_backward_f32's weight-gradient pass = the leading extent of its partials:
 * B * ceil(Ho / 8) * ceil(Wo / 32) (0: invalid sizes). */
int64_t mvbev_thin_conv1_backward_blocks(int64_t B, int64_t Ho, int64_t Wo);

/* dpre [B][Cout][Ho][Wo] fp32 contiguous: the gradient of the pre-activation (the caller has applied the ReLU's
 * mask).  dxw (NULL: not wanted; needs w1) [B][N][Ho][Wo] contiguous:
 *   dxw[b][v][p] = sum_co sum_t w1[co][v][t] dpre[b][co][p - s_t]                              (v < N)
 * partials (NULL: not wanted; needs xw) [blocks][Cout][N][9], npartials >= blocks * Cout * N * 9 values, every
 * one written: the per-workgroup sums of
 *   dw1[co][v][t] = sum_{b, p} dpre[b][co][p] xw[b][v][p + s_t]                                 (v < N)
 * The bias gradient and the coord channels' weight gradient are mvbev_conv3x3_bias_coord_grad_f32's (coord_ch =
 * N); the gradient to the planes is mvbev_warp_views_adjoint of dxw with mvbev_warp_adjoint_plan's plans (C = 1).
 * Fixed summation order, no float atomics: bitwise repeatable.  Errors as the forward. */
int mvbev_thin_conv1_backward_f32(const float* dpre, const float* w1, const float* xw, int nviews, int64_t B,
                                  int64_t Cout, int64_t Ho, int64_t Wo, float* dxw, float* partials, int64_t npartials,
                                  void* stream);

/* dw[co][v][t] for v < N of a [Cout][N + 2][3][3] weight gradient (the two coord channels are not written) = the
 * sums over the nblocks leading slices of partials, in order, in fp64. */
int mvbev_thin_conv1_grad_weight_f32(const float* partials, int64_t nblocks, int nviews, int64_t Cout, float* dw,
                                     void* stream);

/* ---- the front and the closing upsample of ImageProjVariant (added after 12500; mvbev_version() stays 12500) ----
 *
 * image_proj_variant.py:64-88 in one launch: per view F.interpolate(imgs[:, cam], upsample_shape, 'bilinear')
 * (:67), kornia.warp_perspective(img_res, proj_mat, reducedgrid_shape) (:69), and the torch.cat of the N warped
 * 3-channel maps with the coord map (:88):
 *   out[b][3 v + c][r][u]            = the kornia warp (mvbev_warp_perspective_f32's coordinates, blend and zero
 *                                      padding; non-finite coordinates give NaN) of the RESIZED image [Hr][Wr] of
 *                                      view v's channel c, each in-bounds corner of which is PyTorch's
 *                                      align_corners=False bilinear resize of the full-resolution [H][W] image
 *                                      (source index scale (dst + 0.5) - 0.5 clamped at 0 with scale = in / out in
 *                                      fp32, the second tap clamped at the edge): at most 16 taps per sample
 *   out[b][3 N], out[b][3 N + 1]     = the coord values of mvbev_fill_coord_map_f32
 * The resized images are never written.  views[i]: src = view i's image [B][3][H][W] fp32 at element strides
 * src_strides (batch, channel and row strides >= 0, column stride 1: a slice imgs[:, i] of a [B][N][3][H][W] tensor
 * runs without a copy), m = the kornia matrix for a source of Hr x Wr; dst unused.  out: [B][3 N + 2][Ho][Wo] fp32
 * at element strides out_strides (>= 0; NCHW and channels-last outputs hold bitwise-equal values).  flags: 0, or
 * MVBEV_IMG_PROJ_PER_PIXEL (one thread per grid pixel walks the views, instead of one thread per (pixel, view);
 * the same values).  NaN / Inf in the images are outside the contract (an invalid corner is not multiplied).
 * Range: 1 <= nviews <= 16, every tensor below 2^31 elements (else MVBEV_ERR_SHAPE, as an unknown flag; a size <= 0
 * is MVBEV_ERR_RANK, a column stride != 1 or a negative stride MVBEV_ERR_STRIDE, a missing pointer
 * MVBEV_ERR_NULL). */
#define MVBEV_IMG_PROJ_PER_PIXEL 1
int mvbev_img_proj_forward_f32(const mvbev_warp_view* views, int nviews, int64_t B, int64_t H, int64_t W, int64_t Hr,
                               int64_t Wr, int64_t Ho, int64_t Wo, float* out, const int64_t out_strides[4], int flags,
                               void* stream);

/* image_proj_variant.py:92, F.interpolate(map_result, reducedgrid_shape, mode='bilinear') of a one-channel map:
 * x [B][1][h][w] -> y [B][1][Ho][Wo], both fp32 contiguous, PyTorch's align_corners=False taps and order.  Any
 * ratio >= 1 per axis (Ho >= h, Wo >= w; else MVBEV_ERR_SHAPE), integer or not. */
int mvbev_upsample_map_f32(const float* x, int64_t B, int64_t h, int64_t w, int64_t Ho, int64_t Wo, float* y,
                           void* stream);
/* Its adjoint: dx[b][i][j] = the sum over the output pixels whose taps touch (i, j) of weight * dy, gathered per
 * low-resolution pixel in a fixed order (no float atomics: bitwise repeatable).  dy [B][1][Ho][Wo], dx [B][1][h][w],
 * fp32 contiguous; every dx value is written. */
int mvbev_upsample_map_backward_f32(const float* dy, int64_t B, int64_t h, int64_t w, int64_t Ho, int64_t Wo,
                                    float* dx, void* stream);

/* ---- the camera-frame front (added after 12500; mvbev_version() stays 12500) ----
 *
 * main.py:38-40's T.Compose([T.Resize([h, w]), T.ToTensor(), normalize]) of frameDataset.py:127-133 for every view
 * and batch item in one launch, bit for bit: Pillow's 8-bit bilinear resize (two separable passes with 22-bit
 * fixed-point coefficients, horizontal first, acc = 1 << 21; acc += px * coef; clamp(acc >> 22, 0, 255) in int32
 * after each pass), then one table look-up per channel byte for ToTensor + Normalize.
 *   views[i]   view i's decoded frames [B][H][W][3] uint8 ("RGB": pixel stride 3, channel stride 1) with batch
 *              and row strides in bytes (>= 0, any alignment: a slice of a wider buffer is read in place)
 *   bounds_x   [w][2] int32 (first input column, tap count) and coef_x [w][ksx] int32, the horizontal table;
 *   bounds_y   [h][2] and coef_y [h][ksy], the vertical table (device memory; mvdet_amd.frames.resample_table
 *              restates Pillow's precompute_coeffs / normalize_coeffs_8bpc).  Bounds are clamped to the image on
 *              the device.  An axis of equal sizes has the table of one tap of weight 1 << 22: a copy.
 *   lut        [3][256] fp32 (device): the value of byte v in channel c
 *   out        [B][nviews][3][h][w] fp32 at element strides out_strides (>= 0); a wave stores contiguous runs when
 *              the channel stride is 1 (each view in torch's channels_last format) and when the column stride is 1
 *              (NCHW); both hold bitwise-equal values
 * No allocation, no synchronisation.  Range: 1 <= nviews <= 16, 1 <= ksx, ksy <= 64, the output below 2^31
 * elements, and a staged input box that fits 64 KB of LDS at the smallest tile (8 x 32 outputs: downscales up to
 * 7x on both axes, any upscale), else MVBEV_ERR_SHAPE; a size <= 0 is MVBEV_ERR_RANK, a negative stride
 * MVBEV_ERR_STRIDE, a missing pointer MVBEV_ERR_NULL. */
typedef struct mvbev_frame_view {
  const void* src;
  int64_t batch_stride; /* bytes */
  int64_t row_stride;   /* bytes */
} mvbev_frame_view;

int mvbev_frames_resize_normalize_u8(const mvbev_frame_view* views, int nviews, int64_t B, int64_t H, int64_t W,
                                     int64_t h, int64_t w, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                                     const int32_t* bounds_y, const int32_t* coef_y, int ksy, const float* lut,
                                     float* out, const int64_t out_strides[5], void* stream);

/* ---- CLEAR MOD evaluation (added after 12500; mvbev_version() stays 12500) ----
 *
 * The test loop's last step (trainer.py:149-160 -> evaluation/pyeval/CLEAR_MOD_HUN.py) without files, scipy or a
 * host sync per frame.
 *
 * Sync-free detections from the map (mvbev_threshold_points / mvbev_point_nms_ws read their counts on the host):
 *   mvbev_threshold_points_xy   mvbev_threshold_points' ordered compaction, writing the float positions of
 *       trainer.py:103, xy[k] = (row, column) * scale in fp32 ((column, row) when swap_xy), scores[k] and the device
 *       *count.  capacity >= H * W (it cannot overflow), else MVBEV_ERR_SHAPE.
 *   mvbev_point_nms_dev   mvbev_point_nms_ws with K read from the device int32 *K (clamped to [0, capacity]; K = 0:
 *       *count = 0).  points / scores / keep hold capacity entries; workspace >=
 *       mvbev_point_nms_workspace_bytes(capacity, capacity), 4-B aligned.
 *   mvbev_detections_append   copies the *count kept positions points[keep[i]] (i ascending) to buffer[*cursor ...]
 *       ([max_dets][2] fp32), advances *cursor and stores it to *frame_end.  A frame that does not fit sets
 *       *overflow = 1, writes nothing to the buffer and leaves the cursor (*frame_end = *cursor).
 * One workgroup each; enqueued, no allocation, no host sync. */
int mvbev_threshold_points_xy(const float* map, int64_t H, int64_t W, float thres, float scale, int swap_xy,
                              int32_t* count, float* xy, float* scores, int64_t capacity, void* stream);
int mvbev_point_nms_dev(const float* points, const float* scores, const int32_t* K, int64_t capacity,
                        float dist_thres, int64_t top_k, int64_t* keep, int32_t* count, void* workspace,
                        size_t ws_bytes, void* stream);
int mvbev_detections_append(const float* points, const int64_t* keep, const int32_t* count, int64_t capacity,
                            float* buffer, int64_t max_dets, int32_t* cursor, int32_t* frame_end,
                            int32_t* overflow, void* stream);

/* CLEAR_MOD_HUN.py:58-91 for F frames in one launch, one workgroup per frame.  gt [Ng][2] and det [Nd][2] hold the
 * points (device; dtype: both fp32, both fp64, or fp64 GT with fp32 detections), gt_off / det_off [F + 1] int32
 * (device) their CSR offsets by frame.  Per frame: the cost of (GT o, detection e) is d = sqrt(dx^2 + dy^2) in fp64
 * (products and sum rounded separately, correctly rounded sqrt) if d <= td, else 1e6 (so is a NaN / inf distance); the
 * minimum-cost assignment of the smaller side into the larger (scipy's linear_sum_assignment: shortest augmenting
 * paths, fp64 duals, costs evaluated on the fly; ties in a column scan go to the lowest column, so two runs are
 * bitwise equal); a pair counts as matched when d < td (a pair at exactly td is assigned at cost td, not counted).
 *   n_gt, n_det, matched [F] int32; modp_sum [F] fp64 = sum over the frame's matched GT, in GT order, of 1 - d / td;
 *   cost [F] fp64 = the assignment's total cost; match [Ng] int32 (may be NULL) = each GT's frame-local detection, or -1.
 * The host cannot see the frame sizes, so the caller states bounds: max_small >= every frame's min(n_gt, n_det)
 * (<= MVBEV_CLEAR_MOD_MAX_SMALL), max_large >= every frame's max(n_gt, n_det) (<= MVBEV_CLEAR_MOD_MAX_LARGE), else
 * MVBEV_ERR_SHAPE before any launch.  The column state of a frame with up to 2048 columns lives in LDS, that of a
 * larger one in the workspace (>= mvbev_clear_mod_workspace_bytes, 8-B aligned; 0 bytes, and workspace may be NULL,
 * when max_large <= 2048).  A frame that breaks the stated bounds or whose offsets leave [0, Ng] / [0, Nd] is not run:
 * matched = -1 (n_gt = n_det = -1 for bad offsets).  No allocation, no host sync. */
#define MVBEV_CLEAR_MOD_MAX_SMALL 1024
#define MVBEV_CLEAR_MOD_MAX_LARGE (1 << 20)
#define MVBEV_EVAL_F32 0
#define MVBEV_EVAL_F64 1
#define MVBEV_EVAL_GT_F64_DET_F32 2
size_t mvbev_clear_mod_workspace_bytes(int64_t Ng, int64_t Nd, int64_t max_large);
int mvbev_clear_mod_frames(const void* gt, const void* det, int dtype, const int32_t* gt_off, const int32_t* det_off,
                           int64_t F, int64_t Ng, int64_t Nd, int64_t max_small, int64_t max_large, double td,
                           int32_t* n_gt, int32_t* n_det, int32_t* matched, double* modp_sum, double* cost,
                           int32_t* match, void* workspace, size_t ws_bytes, void* stream);

/* ---- the projection on plain channels-last tensors (added after 12500; mvbev_version() stays 12500) ----
 *
 * persp_trans_detector.py:65, :69, :77 as one op (mvdet_amd.ProjectViews): every view's map upsampled to H x W
 * (bilinear, align_corners=False; the identity when h x w == H x W), warped onto the Ho x Wo grid and written into
 * its channel slice of one channels-last tensor, then the two coord channels.  The upsampled maps are never
 * written.  Element kinds: 0 = fp32, 1 = fp16, 2 = bf16; all math is fp32, a 16-bit value is converted exactly at
 * the load and every output value is rounded once (to nearest even) at the store.
 *
 * Forward.  views[i].src: [B][h][w][C] as element strides {batch, 1, row, column} (dst and dst_strides are not read),
 * views[i].m the src_norm <- dst_norm matrix for the H x W source; src_kind the kind of every source.  out:
 * [B][Ho][Wo][Ctot] dense, of out_kind (src_kind, or 0); view i owns channels [i C, (i + 1) C) of a pixel, the coord
 * channels (coord_channels != 0: x then y, the values of mvbev_fill_coord_map_f32) nviews C and nviews C + 1; channels
 * past those, up to Ctot, are not touched.  Coordinates, corners and weights are those of every other warp here
 * (a non-finite coordinate gives NaN, a sample outside the source 0).  H >= h, W >= w, nviews <= 16, and with
 * coord channels Ho, Wo >= 2, else MVBEV_ERR_SHAPE.  Loads and stores use the widest of 16, 8 and 4 bytes (or one
 * element) that the base addresses, the strides, Ctot and C allow; any C >= 1 works.  One launch. */
int mvbev_project_views_cl_forward(const mvbev_warp_view* views, int nviews, int src_kind, int64_t B, int64_t C,
                                   int64_t h, int64_t w, int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* out,
                                   int out_kind, int64_t Ctot, int coord_channels, void* stream);
/* Backward: the adjoint as a deterministic gather over the views' plans (mvbev_warp_adjoint_plan when h x w ==
 * H x W, else mvbev_warp_upsampled_adjoint_plan).  grad_out: [B][Ho][Wo][Ctot] dense, of grad_out_kind; view i reads
 * channels [i C, (i + 1) C).  views[i].grad_src: [B][h][w][C] of grad_src_kind as element strides {batch, 1, row =
 * w * column, column >= C}; NULL: the view is skipped.  grad_out_kind is grad_src_kind or 0.  Every element of a
 * grad_src is written: the sum over its pixel's plan row in CSR order, one fp32 fma per entry (the sum and order of
 * mvbev_warp_views_adjoint with MVBEV_LAYOUT_F32: bitwise its result for fp32), zero for an empty row.  One launch,
 * no atomics. */
typedef struct mvbev_project_views_grad {
  const int32_t* row_ptr;      /* the view's plan */
  const int32_t* col;
  const float* val;
  void* grad_src;
  int64_t grad_src_strides[4];
} mvbev_project_views_grad;
int mvbev_project_views_cl_backward(const void* grad_out, int grad_out_kind, int64_t Ctot,
                                    const mvbev_project_views_grad* views, int nviews, int grad_src_kind, int64_t B,
                                    int64_t C, int64_t h, int64_t w, int64_t Ho, int64_t Wo, void* stream);

/* ---- the weighted multi-plane projection (mvdet_amd.ProjectPlanes; mvbev_version() stays 12500) ----
 *
 *   world_v = sum_d warp_{v,d}(upsample(weight_v[:, d] * feat_v)),  world = cat([world_v for v] + [coord_map])
 *
 * with the layouts, element kinds, coordinates, taps and rounding of mvbev_project_views_cl_*: the sum over the
 * nplanes <= 8 planes is taken inside the gather, so neither the products nor the per-plane warps are written.
 *
 * Forward.  views[i].feat: [B][h][w][C] of src_kind as element strides {batch, 1, row, column >= C} (one batch
 * item's map spans < 2^31 elements); views[i].weight: fp32 [B][nplanes][h][w], dense.  mats: DEVICE fp32
 * [nviews][nplanes][9], plane d of view i's src_norm <- dst_norm matrix for the H x W source (the kernel reads
 * it; the host does not).  out as mvbev_project_views_cl_forward's.  Per tap the term is (a_t * weight[b][d][q_t]) *
 * feat[b][q_t][c] with a_t that entry point's tap coefficient, accumulated in fp32 through the planes in order;
 * with nplanes = 1 and weights of 1.0 the result is bitwise mvbev_project_views_cl_forward's.  A plane whose
 * coordinates are non-finite makes the pixel NaN; a plane that samples outside the source adds 0.  Ho, Wo >= 2.
 * One launch. */
typedef struct mvbev_project_planes_view {
  const void* feat;
  int64_t feat_strides[4];
  const float* weight;
} mvbev_project_planes_view;
int mvbev_project_planes_cl_forward(const mvbev_project_planes_view* views, int nviews, int nplanes,
                                    const float* mats, int src_kind, int64_t B, int64_t C, int64_t h, int64_t w,
                                    int64_t H, int64_t W, int64_t Ho, int64_t Wo, void* out, int out_kind,
                                    int64_t Ctot, int coord_channels, void* stream);
/* Backward, a deterministic gather.  With G_d[c] = sum_e val_e grad_out[b][col_e][i C + c] over row q of plane
 * d of view i (row_ptr [nplanes][h w + 1] indexing col / val: the planes' plans of mvbev_warp_adjoint_plan /
 * mvbev_warp_upsampled_adjoint_plan side by side, each row_ptr offset by where its col / val start), one fp32 fma
 * per entry in CSR order:
 *   grad_feat[b][q][c] = sum_d weight[b][d][q] G_d[c]   (of map_kind, layout as mvbev_project_views_grad.grad_src;
 *                                                        fp32 fmas in plane order, rounded once)
 *   grad_weight[b][d][q] = sum_c feat[b][q][c] G_d[c]   (fp32 [B][nplanes][h][w] dense; per lane over its 16-B
 *                         channel units in ascending order, then the pixel's 8 lanes by a xor butterfly 1, 2, 4)
 * grad_feat NULL / grad_weight NULL: that gradient is not computed (weight / feat is then not read and may be
 * NULL); both NULL: the view is skipped.  feat_strides as grad_feat_strides: {batch, 1, row = w * column,
 * column >= C}.  grad_out_kind is map_kind or 0.  One launch, no atomics, bitwise repeatable. */
typedef struct mvbev_project_planes_grad {
  const int32_t* row_ptr;
  const int32_t* col;
  const float* val;
  const void* feat;
  int64_t feat_strides[4];
  const float* weight;
  void* grad_feat;
  int64_t grad_feat_strides[4];
  float* grad_weight;
} mvbev_project_planes_grad;
int mvbev_project_planes_cl_backward(const void* grad_out, int grad_out_kind, int64_t Ctot,
                                     const mvbev_project_planes_grad* views, int nviews, int nplanes, int map_kind,
                                     int64_t B, int64_t C, int64_t h, int64_t w, int64_t Ho, int64_t Wo,
                                     void* stream);

/* ---- the inference residual tail (added after 12500; mvbev_version() stays 12500) ----
 *
 * mvdet_amd.ResidualTail runs ResNet-18's layer4 (resnet.py:43-75) in eval mode with BatchNorm folded into the
 * 3x3 convs, which are mvbev_conv3x3_bf16x3_ex on MVBEV_LAYOUT_SPLIT_BF16 in and out.  These are the layout and
 * epilogue passes between the fp32 channels-last maps of the backbone and that layout.  All are element-wise over
 * (pixel, 8-channel group) units of 32 B, one launch, no atomics.  C % 8 == 0; M = nviews * B items, item
 * v * B + b = batch item b of view v.
 *
 * Polyphase form of a split-bf16 tensor [M][C/8][h][w]: [4 M][C/8][h2][w2] with h2 = ceil(h / 2), w2 = ceil(w / 2),
 * item 4 m + 2 p + q holding x_pq[r][c] = x[m][2 r + p][2 c + q] and exact zeros where 2 r + p >= h or
 * 2 c + q >= w.  A dilation-4 3x3 conv (padding 4) of x is the dilation-2 conv (padding 2) of each sub-grid on its
 * own: the taps of output (2 r + p, 2 c + q) are x[2 (r + 2 i) + p][2 (c + 2 j) + q], i, j in {-1, 0, 1}, the zero
 * padding included.
 *
 * mvbev_cl_to_split_bf16: views[i].src = [B][h][w][C] of src_kind (0 fp32, 1 fp16, 2 bf16) as element strides
 * {batch, 1, row, column >= C}, 16-B aligned with strides that keep every 8-channel unit 16-B aligned (dst and m
 * of the table are not read); dst: the plain (polyphase == 0) or polyphase layout, hi = bf16(x) to nearest even,
 * lo = bf16(x - hi).  Every unit of dst is written, the zero pads included. */
int mvbev_cl_to_split_bf16(const mvbev_warp_view* views, int nviews, int src_kind, int64_t B, int64_t C, int64_t h,
                           int64_t w, int polyphase, void* dst, void* stream);
/* out = relu(y + identity), the close of a residual block: y split-bf16, plain or (y_polyphase != 0) polyphase,
 * read as hi + lo in fp32; identity an fp32 table as above (one view with B = M for a single tensor); out fp32
 * [M][h][w][C] dense.  ReLU keeps NaN and is torch's otherwise (clamp_min(0)).  next (optional): the same values
 * split as by mvbev_cl_to_split_bf16 of out, plain or (next_polyphase != 0) polyphase with its zero pads — the next
 * block's conv input without a conversion launch. */
int mvbev_res_close_f32(const void* y, int y_polyphase, const mvbev_warp_view* identity, int nviews, int64_t B,
                        int64_t C, int64_t h, int64_t w, float* out, void* next, int next_polyphase, void* stream);
/* The polyphase layout [4 M][C/8][h2][w2] back to the plain [M][C/8][h][w] (a dilation-4 conv's output for the
 * dilation-1 conv after it): a permutation copy of the units; the pads are not read. */
int mvbev_split_polyphase_to_plain(const void* src, int64_t M, int64_t C, int64_t h, int64_t w, void* dst,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVBEV_H_ */
