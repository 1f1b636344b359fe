/*
 * wsdl_hip.h - C ABI of libwsdl_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * weakly-supervised segmentation hot path of alexncoleman/WeaklySupervisedDL.
 *
 * The reference has no FFI of its own: every operator below is a chain of PyTorch ATen ops reached
 * from Python (reference file:line cited per entry point, relative to the reference root).  These
 * entry points are what a binding for that path binds instead; INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - every tensor is fp32, contiguous NCHW unless a *_bs (batch stride, in elements) says otherwise;
 *     labels are int64 (the host API's dtype), masks uint8;
 *   - all pointers are caller-owned DEVICE pointers; the library allocates nothing persistent,
 *     scratch is an explicit caller-sized workspace (see the *_workspace functions);
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant across
 *     streams, and performs no host synchronisation: launches can be captured into a hipGraph;
 *   - return value 0 = OK, negative = WSDL_E* ; wsdl_last_error() returns a thread-local message.
 *     Geometry is validated on the host before any launch; a rejected call launches nothing.
 */
#ifndef WSDL_HIP_H
#define WSDL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* wsdl_stream_t; /* hipStream_t */

enum {
    WSDL_OK = 0,
    WSDL_EINVAL = -1,      /* bad geometry / null pointer / unsupported size */
    WSDL_EHIP = -2,        /* a HIP runtime call failed (message holds hipGetErrorString) */
    WSDL_EWORKSPACE = -3   /* workspace too small */
};

const char* wsdl_last_error(void);
/* Launch trace (diagnostic): wsdl_launch_trace(1) makes the convolution entry points describe every launch they choose -
 * kernel form and tile, arithmetic, K slices, XCD order, column bands, pixel splits, grid - into a per-thread string;
 * wsdl_last_launches() returns this thread's descriptions since its previous call ("; "-separated, valid until the next
 * call) and clears them.  Off (default): one relaxed load per launch site.  The full-size parity tests use it to name
 * the configuration each comparison against the float64 oracle went through. */
int wsdl_launch_trace(int on);
const char* wsdl_last_launches(void);
int wsdl_version(void);               /* 10000*major + 100*minor + patch */
const char* wsdl_target_arch(void);   /* "gfx950" */

/* Process-wide options.  Each is an int read with relaxed atomic loads by every entry point: a call that runs while another
 * host thread sets an option sees the old or the new value, never a torn one.  wsdl_set_option is serialised and REFUSES
 * (WSDL_EINVAL) while any host thread is recording a launch plan - a plan freezes the tile choices of the option set it was
 * recorded under.  Changing "conv_split" / "conv_arith" changes what the weight layout buffers hold: re-run
 * wsdl_conv2d_prep_weights afterwards (callers that cache layouts key them on the option set: ops.LAYOUT_EPOCH).
 *   conv_arith     1*  arithmetic of the split kernels: 1 = fp16x2 (three 16-bit MFMAs per fp32 product, per-tensor
 *                      power-of-two scales from the amax arguments), 0 = bf16x3 (six MFMAs, no scales),
 *                      2 = fp16x2 with the low piece carried at 2^11 and the cross products in a second accumulator
 *                      (forward / input gradient; the RANGE GUARD: a region of a tensor keeps 22 bits down to 2^-29 of the
 *                      tensor's maximum instead of 2^-18 and is exact to 2^-50 of it instead of 2^-39 - same three MFMAs, 64
 *                      more registers per lane, which ends the co-residency with the weight-gradient workgroups: -6.6 % img/s
 *                      on the training step, profiles/r04_notes.md; use it when gradients span more than 2^25 inside one tensor)
 *   conv_split     1*  0 = forward / input-gradient convolutions on the exact-fp32 MFMA kernels everywhere
 *   wgrad_split    1*  0 = weight gradients on the exact-fp32 MFMA kernels everywhere
 *   tile_threshold 400* workgroups below which the half-size pixel tile is used
 *   xcd_map        1*  XCD-aware tile order of the split kernels (0 off, 1 auto, 10 + py forces py row groups)
 *   wgrad_min_tiles 1*  which shapes the fp16x2 weight-gradient kernel takes: from this many 128-wide N tiles on (rounds 2-5: 6 - from
 *                      one tile on the layer2 1x1 kernels were 20-30 % faster and the step 1 % slower: pre-split, reduce and amax
 *                      launches; round 6, with the pre-split and the maxima coming from the producers: +0.5-0.9 % on the step)
 *   wgrad_xcd      1*  split weight-gradient kernel: XCD-aware tile order (1 contiguous eighths, 2 in 2x2 blocks); bit-identical,
 *                      -1.4 % on the kernel sweep, +0.4 % on the step (half the traffic past L2 for the kernels beside it)
 *   group_tps10   45*  wsdl_conv2d_fwd_group: taps per K slice in tenths (45: a 9-tap problem in 2 slices, the others whole; 20 -
 *                      round 5's default: 4 and 2 slices, eight streams; same box 575.7 us at 45 against 638.6 at 20)
 *   range_sentinel 0*  1 = the amax arguments of wsdl_bn_train_fwd / _bwd are (max, ~min channel maximum) pairs (wsdl_range_check)
 *   bn_resident    1*  channel-resident fused BatchNorm kernels where a channel fits one workgroup's registers (0 off, 1 = from
 *                      64 channels, n > 1 = from n channels; measured: resident wins at every channel count of the networks)
 *   bn_wide_c    512*  resident BatchNorm kernels as 1024 threads x 4 float4 (instead of 256 x 16) up to this channel count
 *                      (half of it for the backward): 16 waves per CU loading at once where one workgroup per channel would
 *                      leave a CU with 4 - forward -20..23 %, backward -7 % at 256 channels (profiles/r03_bn_kernels.txt)
 *   conv_il        1*  256x128 forward / input-gradient form (all three entry points): steady-state K loop with every wave's MFMAs
 *                      and staging instructions interleaved (branch-free body + scheduling directives) - both waves of a SIMD run
 *                      the same phase, so staging otherwise never overlaps the other wave's MFMAs; bit-identical, 2-8 % faster
 *                      per launch in isolation, +0.5 % on the (power-bound) step
 *   wgrad_blocks 768*  target workgroups of a weight-gradient launch
 *   wgrad_direct   1*  fp16x2 weight-gradient kernel with the x operand's MFMA fragments loaded straight from global memory (no LDS, no
 *                      lane exchange for x; dY double-buffered in LDS, one barrier per chunk) where OW % 32 == 0, stride 1 and every
 *                      tap's column shift is a multiple of 4 elements (1x1, dilation 4 / 12 / 24 / 36): 7-10 % faster there, bit-identical;
 *                      0 = the LDS-staged kernel everywhere
 *   wgrad_dyraw    1*  the direct-fragment kernel reads dY as fp32 and splits it while staging (no dy_split16 pre-pass) for 1x1 convolutions
 *                      with at most 10 N tiles (7-11 % faster there); 2 = for every launch of that kernel (3x3: 7-21 % slower), 0 = never
 *   wgrad_chan_scale 0* the range guard of the weight gradient (conv_arith = 2 is the forward / input gradient's): the fp16x2 weight-gradient
 *                      kernels scale x and dY by one power of two per CHANNEL instead of per tensor - a channel is a row / a column
 *                      of that GEMM's output (K = pixels), so the inverse scales go onto the result's rows and columns: exact, no
 *                      second accumulator set.  A pre-pass takes the per-channel maxima (one more read of x and dY per layer)
 *   stem_kernel    1*  7x7 stride-2 convolution of 3 -> 64 channels (ResNet's conv1) on its own kernel: input patch and all weights
 *                      in LDS, fp32 MFMA (0: the generic fp32 implicit-GEMM kernel, the A/B partner)
 *   ksplit_target 512* / ksplit_max 8* / ksplit_min_chunks 4*  small grids (CAM path at B=8): workgroups aimed at by the K split,
 *                      most K slices, fewest 32-deep chunks per slice
 *   layercam_tail_mod 32*  LayerCAM epilogue: the last hw % n pixels of a map are summed over the channels the way ATen's CPU sum
 *                      handles its scalar columns (four interleaved streams), all others by its four-level cascade - the epilogue
 *                      is bit-identical to the reference's torch-CPU arithmetic on identical inputs.  32 = torch built for AVX-512
 *                      run on 1-12, 24 or 32 threads (the fixtures: torch.set_num_threads(4)), 16 = an AVX2 torch, 0 = the
 *                      cascade for every pixel.  torch-CPU's own result depends on its THREAD COUNT: ATen splits the
 *                      columns of the sum over its threads and the thread left with fewer than a vector's worth takes the
 *                      scalar path, so no single setting reproduces every reference run - with 16 threads (the GPU boxes'
 *                      default) 32 leaves 2 of 196 values of a 1024 x 14 x 14 sum one ulp off and 0 leaves 6 of 784 (28 x 28) and 9
 *                      of 49 (7 x 7); pin the reference's thread count (1-12) when bit-exact CAM values are compared
 * (Options measured slower and removed in round 3: conv_glds - weights by LDS-DMA; wgrad_wide - 8-pixel-run staging of x;
 *  wgrad_tile64 - 64-row weight-gradient tiles; occupancy_cap.  Figures: profiles/r02_notes.md.  Round 4: t256_bk32 - K chunks of 32
 *  in the 256x128 form (1-2.6 % slower per step); wgrad_direct = 2 - the direct-fragment weight gradient for misaligned taps (0-7 %
 *  slower, spills); conv_mfma16 / wgrad_mfma16 = 0 - the 32x32x16 MFMA shape in the K-chunk-32 forward forms and in the fp16x2 weight
 *  gradient (2.2 % / 2 % slower on the step; v_mfma_f32_16x16x32_f16 is what those kernels run on).
 *  Rounds 5 and 6, removed whole: bn_coop / bn_coop_wide - several workgroups per channel in the resident BatchNorm kernels, waiting
 *  for each other's partial sums (0.3 % of the step, off since it was written; profiles/r05_notes.md); the deferred slab reductions
 *  of the weight gradients - one launch for all layers' slabs at the end of the backward pass (1.2 % slower in every grouping;
 *  profiles/r06_notes.md); the timing-only and lane-pairing experiment builds of the split kernels (profiles/r06_notes.md).
 *  One-off experiment switches hard-wired to their defaults (profiles/r05_notes.md, profiles/r06_notes.md): xcd_rowfast (off),
 *  ms_rowfast (on), ms_py (4 row groups), group_interleave (on), wgrad_force_s (off), wgrad_bk (16), tile_img_major (grouped forward
 *  only), bk32, split_bk32, ksplit_big, tile256, tile64, col_bands, stem_wgrad, wgrad_imbalance_split (all on).)
 * (* = default). */
int wsdl_set_option(const char* name, int value);

/* ---- per-kernel-class timing (bench.py roofline leg) --------------------------------------
 * When enabled every launch of the instrumented classes is bracketed by hipEventRecord on the
 * launch stream.  wsdl_prof_collect synchronises the events and returns, per class, the number of
 * launches, summed milliseconds and summed algorithmic work (flops for conv classes, bytes else).
 * Classes are kernel instantiations, so a class lines up with one row of `rocprofv3 --stats`. */
enum { WSDL_PROF_IGEMM_128x128_A = 0,  /* conv_igemm_fast_kernel<128,128,2,16> (forward + dgrad launches) */
       WSDL_PROF_IGEMM_128x128_U = 1,  /* conv_igemm_kernel<128,128,2,false> (K not a multiple of 16)     */
       WSDL_PROF_IGEMM_128x64_A = 2, WSDL_PROF_IGEMM_128x64_U = 3,
       WSDL_PROF_IGEMM_64x256_A = 4, WSDL_PROF_IGEMM_64x256_U = 5,
       WSDL_PROF_IGEMM_64x128_A = 6, WSDL_PROF_IGEMM_64x128_U = 7,
       WSDL_PROF_WGRAD_128x128 = 8,    /* conv_wgrad_kernel<128,128,2> */
       WSDL_PROF_WGRAD_64x128 = 9,     /* conv_wgrad_kernel<64,128,1>  */
       WSDL_PROF_WGRAD_FAST_128x128 = 10,  /* conv_wgrad_fast_kernel<128,128,2,16> (and its 128x64 / 64x128 / 64x64 forms) */
       WSDL_PROF_PAIRWISE = 11, WSDL_PROF_LAYERCAM = 12,
       /* split kernels (three fp16 / six bf16 MFMAs per fp32 product; work counted in fp32-equivalent FLOPs);
        * the last template argument is the arithmetic (1 = fp16x2, 0 = bf16x3) */
       WSDL_PROF_SPLIT_128x128 = 13,   /* conv_igemm_split_kernel<128,128,2,16,256,AR> (forward + dgrad launches) */
       WSDL_PROF_SPLIT_128x64 = 14, WSDL_PROF_SPLIT_64x256 = 15, WSDL_PROF_SPLIT_64x128 = 16,
       WSDL_PROF_WGRAD_SPLIT32 = 17,   /* conv_wgrad_split32_kernel<128,128,AR> */
       WSDL_PROF_SPLIT_256x128 = 18,   /* conv_igemm_split_kernel<256,128,4,32|16,512,AR> */
       WSDL_PROF_STEM = 19,            /* stem_conv7x7s2_kernel */
       WSDL_PROF_WGRAD_SPLIT16D = 20,  /* conv_wgrad_split16d_kernel<MODE, DYRAW> (x fragments straight from global memory); class 17 is then
                                          the LDS-staged conv_wgrad_split16_kernel / conv_wgrad_split32_kernel.  Both brackets include the
                                          launch's dy_split16 pre-pass where there is one */
       WSDL_PROF_SPLIT_GROUP = 21,     /* conv_igemm_split_group_kernel<256,128,4,16,512,AR,false>: several forward convolutions, one launch */
       WSDL_PROF_SPLIT_MULTI = 22,     /* conv_igemm_split_kernel<256,128,4,16,512,AR,false,true>: several input gradients, one accumulator */
       WSDL_PROF_NCLASSES = 23 };
const char* wsdl_prof_class_name(int cls);
int wsdl_prof_enable(int on);
int wsdl_prof_collect(int cls, long long* launches, double* total_ms, double* total_work,
                      double* total_work_executed /* work minus the skipped all-padding K-chunks */,
                      double* total_bytes /* algorithmic HBM bytes: every operand read once, result written once */);
int wsdl_prof_reset(void);

/* ---- profiler ranges (roctx) ----------------------------------------------------------------
 * Named host-side ranges for `rocprofv3 --marker-trace`: wsdl_range_enable(1) loads librocprofiler-sdk-roctx.so (dlopen; the
 * library does not link against it) and from then on wsdl_range_push / _pop forward to roctxRangePushA / roctxRangePop, and
 * every launch of an instrumented kernel class (the classes above) sits inside a range carrying the class name.  Disabled
 * (the default) all three cost one branch.  Returns 0, or WSDL_EINVAL when the roctx library cannot be loaded.
 * The reference has no tracing of any kind: this is the build's addition. */
int wsdl_range_enable(int on);
int wsdl_range_push(const char* name);
int wsdl_range_pop(void);

/* ---- convolution: implicit GEMM on the matrix cores -------------------------------------------
 * Arithmetic paths, all at fp32-level accuracy (tools/conv_accuracy.py, tests/test_hip_ops.py measure them against fp64):
 *   fp32 : v_mfma_f32_32x32x2_f32, exact fp32 fma chains;
 *   split: every fp32 operand is split exactly into 16-bit pieces and a product is a few 16-bit MFMA partial products
 *          accumulated in fp32 - used whenever the contracted channel count is a multiple of 16 and kh*kw <= 9
 *          (wsdl_set_option("conv_split", 0) / ("wgrad_split", 0) select the fp32 kernels everywhere):
 *            fp16x2 (default): x*s = h + l in fp16 (22 bits), three v_mfma_f32_32x32x16_f16 per product; s is a power of
 *                    two per tensor, derived in the kernel from the `*_amax` device scalars (>= max|tensor|, e.g. from
 *                    wsdl_bn_train_fwd / wsdl_amax), which are therefore REQUIRED (non-NULL) for these launches;
 *            bf16x3 ("conv_arith" 0): x = h + m + l in bf16 (24 bits), six v_mfma_f32_32x32x16_bf16, amax unused.
 * Replaces the ATen conv2d forward / input-gradient / weight-gradient reached from
 *   torchvision ResNet-50 and DeepLabV3 convs called at TraditionalModel/ClassificationModel.py:29-33,
 *   TraditionalModel/SegmentationModel.py:102,110, TraditionalModel/AlternatingDirectionCutLoss.py:697-703,
 *   and the class-logit backward at TraditionalModel/LayerCAM.py:48.
 * Square kernels, one stride / padding / dilation for both spatial dims, groups = 1.
 *   OH = (H + 2*pad - dil*(kh-1) - 1)/stride + 1 (same for OW).                                   */

/* Re-layout w[Cout][Cin][kh][kw] for the kernels.  The layout buffers are opaque to the caller; their size
 * comes from wsdl_conv2d_weight_layout_bytes (dgrad = 0: forward layout, 1: input-gradient layout):
 *   plain  (fp32 MFMA kernels)      : wt_fwd[(tap*Cin+ci)][Cout], wt_dgrad[(tap*Cout+co)][Cin]  fp32;
 *   split  (used when the contracted channel count % 16 == 0 and kh*kw <= 9):
 *            [(k/16)][row][piece][k%16] 16-bit pieces (fp16x2: w * 2^e = h + l, 4 bytes per weight; bf16x3: h + m + l,
 *            6 bytes per weight) + a 16-byte trailer holding max|w| (the scale the kernels derive 2^e from).
 * *is_plain (optional) tells which one the current options select; for a plain 1x1 kernel the dgrad layout
 * equals w itself.  Either destination of prep_weights may be NULL. */
size_t wsdl_conv2d_weight_layout_bytes(int Cout, int Cin, int kh, int kw, int dgrad, int* is_plain);
int wsdl_conv2d_prep_weights(const float* w, void* wt_fwd, void* wt_dgrad,
                             int Cout, int Cin, int kh, int kw,
                             const float* w_amax /* optional device scalar max|w| (wsdl_multi_amax); NULL: reduced here */,
                             wsdl_stream_t stream);

/* y = act( scale[co]*conv(x) + shift[co] + residual ), any of scale/shift/residual may be NULL
 * (scale NULL = 1, shift NULL = 0).  relu != 0 applies max(.,0).  x_bs / y_bs / res_bs: batch strides
 * in elements (0 = dense).  Folded eval-mode BatchNorm, conv bias and the Linear layer (a 1x1 conv on
 * a 1x1 map) all go through scale/shift. */
int wsdl_conv2d_fwd(const float* x, const void* wt_fwd, float* y,
                    int B, int Cin, int H, int W, int Cout, int kh, int kw,
                    int stride, int pad, int dil,
                    const float* scale, const float* shift, const float* residual, int relu,
                    long long x_bs, long long y_bs, long long res_bs,
                    const float* x_amax /* device scalar >= max|x| (fp16x2 split launches; else may be NULL) */,
                    float* y_amax /* optional: atomicMax of max|y| into a ZEROED device scalar */,
                    void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* The split layouts of MANY convolutions in one launch (the re-layout after an optimiser step).  Entries must be convolutions
 * whose forward AND dgrad layouts are split layouts (wsdl_conv2d_weight_layout_bytes: plain = 0 for both; kh*kw <= 9) under the
 * fp16x2 arithmetic; w_amax as in wsdl_conv2d_prep_weights but REQUIRED.  `desc` is a DEVICE array of n entries, block_begin =
 * the running sum of grid_x * grid_y with grid_x = ceil(Cin / 32), grid_y = ceil(Cout / 32); total_blocks = its final value. */
typedef struct wsdl_prep_desc {
    const float* w;          /* [Cout][Cin][taps] */
    void* wt_fwd;            /* may be NULL */
    void* wt_dgrad;          /* may be NULL */
    const float* w_amax;     /* device scalar >= max|w| */
    int Cout, Cin, taps, grid_x;
    int block_begin, reserved;
} wsdl_prep_desc;
int wsdl_conv2d_prep_weights_multi(const wsdl_prep_desc* desc, int n, int total_blocks, wsdl_stream_t stream);

/* Optional scratch for forward / dgrad: grids too small to fill 256 CUs (small batches of small maps) are split
 * along K into slabs summed in fixed order.  Returns 0 when the geometry does not benefit; ws may be NULL. */
size_t wsdl_conv2d_igemm_workspace(int B, int Cin, int H, int W, int Cout, int kh, int kw,
                                   int stride, int pad, int dil, int dgrad);

/* dx = conv_transpose(dy, w)  (+ dx if accumulate).  dy is (B,Cout,OH,OW) with batch stride dy_bs.
 * acc_mask (optional, with accumulate): bit e % 8 of byte e / 8 says whether element e of the value already in dx counts -
 * dx then holds a bottleneck block's output gradient and the mask is the block's final ReLU as written by
 * wsdl_bn_train_fwd(relu_mask): dx = dgrad + [y > 0] * dx, the identity branch's gradient without a tensor of its own. */
int wsdl_conv2d_dgrad(const float* dy, const void* wt_dgrad, float* dx,
                      int B, int Cin, int H, int W, int Cout, int kh, int kw,
                      int stride, int pad, int dil, int accumulate, const uint8_t* acc_mask,
                      long long dy_bs, const float* dy_amax, void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* The input gradient of n (2..4) convolutions that read the SAME input, in one launch:
 *   dx = [accumulate: dx +] sum_i dgrad(dy[i], wt_dgrad[i])      (1x1 / 3x3, stride 1, padding dil*(k-1)/2: 'same')
 * - the ASPP head of DeepLabV3, whose 2048-channel input feeds a 1x1 and three dilated 3x3 branches (torchvision's
 * ASPP.forward; reference TraditionalModel/SegmentationModel.py:85 builds it) and whose input gradient the reference
 * obtains as four conv-backward calls and three tensor adds.  The output tile accumulates over all sources' taps in
 * registers (per-source power-of-two scales, the accumulators are moved between them exactly) and is stored once.
 * dy / wt_dgrad / dy_amax / k / dil / dy_bs are HOST arrays of n entries (dy_bs may be NULL: dense).  Source 0 decides the
 * output-column bands of the tap skipping: pass the smallest dilation > 1 first.  wsdl_conv2d_dgrad_multi_ok says whether a
 * geometry is served (else: chain wsdl_conv2d_dgrad calls with accumulate = 1). */
/* n (2..4) forward convolutions of ONE input in one launch - ASPP's 1x1 and three dilated 3x3 branches (torchvision's
 * ASPP.forward, built by reference TraditionalModel/SegmentationModel.py:85): y[i] = conv(x, w[i]), 1x1 / 3x3, stride 1, 'same'
 * padding, raw outputs (the BatchNorm kernels follow).  The branches execute 1..9 taps per pixel tile (padding taps are
 * skipped): launched one by one each ends with idle CUs behind its longest tiles; here the workgroups of all problems form
 * one grid, heaviest problem first, tiles of more than two taps cut into K slices (slabs in the workspace + the fixed-order
 * reduce).  wt_fwd / y / k / dil / y_bs: HOST arrays of n entries (y_bs may be NULL: dense). */
int wsdl_conv2d_fwd_group_ok(int n, int B, int Cin, int H, int W, int Cout);
size_t wsdl_conv2d_fwd_group_workspace(int n, const int* k, const int* dil, int B, int Cin, int H, int W, int Cout);
int wsdl_conv2d_fwd_group(int n, const float* x, const void* const* wt_fwd, float* const* y, const int* k, const int* dil,
                          int B, int Cin, int H, int W, int Cout, long long x_bs, const long long* y_bs,
                          const float* x_amax, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_conv2d_dgrad_multi_ok(int n, int B, int Cin, int H, int W, int Cout);
int wsdl_conv2d_dgrad_multi(int n, const float* const* dy, const void* const* wt_dgrad, const float* const* dy_amax,
                            const int* k, const int* dil, const long long* dy_bs, float* dx, int B, int Cin, int H, int W,
                            int Cout, int accumulate, wsdl_stream_t stream);

/* dw[Cout][Cin][kh][kw] = sum_{b,oh,ow} dy * x_shifted  (+ dw if accumulate).  Split over pixel
 * ranges into fp32 slabs in `ws`, summed in fixed order by a second kernel (bitwise reproducible). */
size_t wsdl_conv2d_wgrad_workspace(int B, int Cin, int H, int W, int Cout, int kh, int kw,
                                   int stride, int pad, int dil);
int wsdl_conv2d_wgrad(const float* x, const float* dy, float* dw,
                      int B, int Cin, int H, int W, int Cout, int kh, int kw,
                      int stride, int pad, int dil, int accumulate,
                      long long x_bs, long long dy_bs, const float* x_amax, const float* dy_amax,
                      void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* The weight gradient with PER-CHANNEL operands (round 6; both optional, NULL = as wsdl_conv2d_wgrad):
 *   x_chan_amax[Cin] / dy_chan_amax[Cout]: one maximum per channel of x / dY, as the channel-resident BatchNorm kernels publish
 *     them (wsdl_bn_train_fwd / _bwd chan_amax).  The fp16x2 kernels then scale each channel by its OWN power of two - exact (a
 *     channel is a row / column of this GEMM's output) and the range guard of the weight gradient for nothing: a channel 2^30
 *     below the tensor's maximum keeps its 22 bits.  "wgrad_chan_scale" = 1 takes missing maxima with a pre-pass instead.
 *   dy_presplit: dY already as the kernel's fp16 (high, low) rows [ceil(P / 32)][Cout][128 B], written by the BatchNorm backward that
 *     produced dY (wsdl_bn_train_bwd dy_presplit) with the scales of dy_chan_amax: dy_split16_kernel (one more read and write of
 *     dY per layer, 24 launches per training step) does not run.  wsdl_conv2d_wgrad_presplit_bytes: the buffer's size for a
 *     geometry, 0 where the weight gradient would not use it. */
size_t wsdl_conv2d_wgrad_presplit_bytes(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dil);
int wsdl_conv2d_wgrad_ex(const float* x, const float* dy, float* dw, int B, int Cin, int H, int W,
                         int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                         long long x_bs, long long dy_bs, const float* x_amax, const float* dy_amax,
                         const float* x_chan_amax, const float* dy_chan_amax, const void* dy_presplit, void* ws,
                         size_t ws_bytes, wsdl_stream_t stream);

/* out = max|x| over B images of per_image contiguous floats (batch stride x_bs elements, 0 = dense); zero_first != 0
 * zeroes `out` first (else the caller passes a zeroed scalar).  For tensors whose producer did not publish an amax
 * (network input, concatenations, dropout outputs).  wsdl_multi_amax: n tensors in one launch - ptrs / counts are
 * DEVICE arrays of n pointers / element counts, out[n] is zeroed first (every conv weight after the optimiser step). */
int wsdl_amax(const float* x, int B, long long per_image, long long x_bs, float* out, int zero_first,
              wsdl_stream_t stream);
int wsdl_multi_amax(const float* const* ptrs, const long long* counts, int n, float* out, wsdl_stream_t stream);

/* dbias[co] = sum_{b,hw} dy  (classifier[4] / fc bias gradient). */
int wsdl_bias_grad(const float* dy, float* dbias, int B, int C, int HW, long long dy_bs,
                   int accumulate, wsdl_stream_t stream);

/* ---- BatchNorm2d (train-mode batch statistics; torchvision BN inside the models above) ------ */
size_t wsdl_bn_workspace(int C);
/* y = act( (x-mean)*invstd*gamma + beta + residual ); saves mean / invstd (biased var), updates
 * running_mean / running_var (unbiased var, momentum) when they are non-NULL. */
int wsdl_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* y,
                      float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                      float momentum, float eps, int B, int C, int HW,
                      const float* residual, int relu, long long y_bs,
                      float* y_amax /* optional: atomicMax of max|y| into a ZEROED device scalar */,
                      uint8_t* relu_mask /* optional (relu, HW % 8 == 0, y_bs % 4 == 0): B*C*HW/8 bytes, bit e%8 of byte
                                            e/8 = [y > 0] for the dense element index e - for relu = 3 of the backward */,
                      void* ws, size_t ws_bytes,
                      float* chan_amax /* optional [C]: max|y| per CHANNEL (a plain store by the channel's workgroup; wants y_amax and
                                          wsdl_bn_channel_resident(B, C, HW, 0)) - the per-channel scales of the weight gradient that
                                          reads y as its x operand (wsdl_conv2d_wgrad_ex) */,
                      wsdl_stream_t stream);
/* 1 when (B, C, HW) runs the channel-resident kernel (one workgroup holds a whole channel in registers: what chan_amax /
 * dy_presplit need), forward (backward = 0) or backward (1), under the current options. */
int wsdl_bn_channel_resident(int B, int C, int HW, int backward);
/* Backward of the above.  relu = 1: the ReLU mask is read from the forward output y (needed when a residual was
 * added); relu = 2: the mask is recomputed from x - y = fma(x - mean, invstd*gamma, beta), the forward's own pinned
 * expression - so y is neither read nor needs keeping (y may be NULL, beta is required); relu = 3: the mask is read from
 * the bits the forward wrote (relu_mask: 1/32 of y's bytes - the residual layers' backward reads four tensor streams
 * instead of five; same result bit for bit as relu = 1); relu = 0: no activation.
 * dres (optional) receives the masked upstream gradient (the residual branch's gradient). */
int wsdl_bn_train_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* beta,
                      const float* save_mean, const float* save_invstd,
                      float* dx, float* dgamma, float* dbeta, float* dres,
                      int B, int C, int HW, int relu, int accumulate_param_grads,
                      long long dy_bs, long long y_bs,
                      float* dx_amax /* optional: atomicMax of max|dx| into a ZEROED device scalar */,
                      const uint8_t* relu_mask /* relu = 3 */,
                      void* ws, size_t ws_bytes,
                      float* chan_amax /* optional [C]: max|dx| per channel (as for the forward; wsdl_bn_channel_resident(.., 1)) */,
                      void* dy_presplit /* optional: dx ALSO as the fp16 (high, low) rows the producing convolution's weight gradient
                                           reads ([B*HW / 32][C][128 B], each channel scaled by the power of two of its chan_amax;
                                           size: wsdl_conv2d_wgrad_presplit_bytes) - the channel's workgroup holds it in registers
                                           anyway.  Wants chan_amax and B*HW % 32 == 0 (dx itself is always dense) */,
                      wsdl_stream_t stream);
/* eval-mode fold: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale (fed to wsdl_conv2d_fwd). */
int wsdl_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, float eps, float* scale, float* shift, int C,
                 wsdl_stream_t stream);
/* y = act(scale[c]*x + shift[c]) - a stand-alone eval-mode BatchNorm2d (scale / shift from wsdl_bn_fold) or a
 * stand-alone ReLU (scale = shift = NULL); the models run both fused behind the convolution instead. */
int wsdl_affine_act_fwd(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                        int relu, wsdl_stream_t stream);
/* backward of y = act(scale*conv + shift + res) wrt conv: dconv = dy*[y>0]*scale ; dres = dy*[y>0] */
int wsdl_affine_act_bwd(const float* dy, const float* y, const float* scale, float* dconv, float* dres,
                        int B, int C, int HW, int relu,
                        float* dconv_amax /* optional: atomicMax of max|dconv| into a ZEROED device scalar */,
                        wsdl_stream_t stream);

/* ---- pooling / resampling / elementwise ----------------------------------------------------- */
/* MaxPool2d(3, stride 2, pad 1) as in ResNet's stem; argmax (0..8, first max wins) kept as uint8 */
int wsdl_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* argmax, int BC, int H, int W,
                          wsdl_stream_t stream);
int wsdl_maxpool3x3s2_bwd(const float* dy, const uint8_t* argmax, float* dx, int BC, int H, int W,
                          wsdl_stream_t stream);
/* AdaptiveAvgPool2d(1) */
int wsdl_global_avgpool_fwd(const float* x, float* y, int BC, int HW, wsdl_stream_t stream);
int wsdl_global_avgpool_bwd(const float* dy, float* dx, int BC, int HW, int accumulate,
                            wsdl_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False): (BC,h,w) -> (BC,H,W).  y_bs/C: output may be a
 * channel slice of a wider tensor (C planes per image, batch stride y_bs elements; 0 = dense). */
int wsdl_bilinear_fwd(const float* x, float* y, int B, int C, int h, int w, int H, int W,
                      long long y_bs, wsdl_stream_t stream);
int wsdl_bilinear_bwd(const float* dy, float* dx, int B, int C, int h, int w, int H, int W,
                      long long dy_bs, wsdl_stream_t stream);
/* Dropout: mask is uint8 0/1.  If gen_mask != 0 the mask is drawn (counter hash of seed, element
 * index) and written; else it is read (injected mask, parity tests).  y = x*mask/(1-p).
 * seed_dev (optional): a device-resident call counter mixed into the seed - a captured (hipGraph) launch replays with a
 * frozen host `seed`, the counter (bumped on the stream by the caller) keeps the masks changing. */
int wsdl_dropout_fwd(const float* x, float* y, uint8_t* mask, size_t n, float p,
                     unsigned long long seed, int gen_mask, const unsigned long long* seed_dev,
                     wsdl_stream_t stream);
int wsdl_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, size_t n, float p,
                     wsdl_stream_t stream);
/* y = a + b (optionally relu), y = alpha*x, strided channel-slice copy */
int wsdl_add(const float* a, const float* b, float* y, size_t n, int relu, wsdl_stream_t stream);
int wsdl_scale_by_device_scalar(const float* x, const float* s, float* y, size_t n, wsdl_stream_t stream);
int wsdl_copy_planes(const float* src, float* dst, int B, int C, int HW, long long src_bs,
                     long long dst_bs, wsdl_stream_t stream);

/* ---- BASNet saliency inference (csrc/basnet.hip; reference PretrainedBasnetModel/model/BASNet.py, RunInference.py) ----
 * The network's convolutions are wsdl_conv2d_fwd with BatchNorm folded into scale / shift.  Its bridge and decoder
 * convolutions carry a bias in front of their BatchNorm (nn.Conv2d default bias=True, BASNet.py:144-234):
 * shift = beta + (bias - rm) * scale, scale = gamma / sqrt(rv + eps) (wsdl_bn_fold without the bias otherwise). */
int wsdl_bn_fold_bias(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      const float* bias, float eps, float* scale, float* shift, int C, wsdl_stream_t stream);
/* nn.MaxPool2d(2, 2, ceil_mode=True) (BASNet.py:124,130; RefUnet pool1..4, :19-37): (B,C,H,W) -> (B,C,ceil(H/2),ceil(W/2)),
 * the last window of an odd side clipped; NaN propagates as in ATen.  x_bs / y_bs: batch strides (channel slices of a wider
 * tensor; 0 = dense). */
int wsdl_maxpool2x2_ceil_fwd(const float* x, float* y, int B, int C, int H, int W, long long x_bs, long long y_bs,
                             wsdl_stream_t stream);
/* A side output: logits = Conv2d(Cin, 1, 3, padding=1)(x) + bias (+ residual), then (y non-NULL) y = sigmoid(bilinear
 * up-sample by s of the logits) - outconv{b,6,5,4,3,2,1} + upscore{6,5,4,3,2} + F.sigmoid (BASNet.py:245-251,323-344);
 * with residual = outconv1's logits and s = 1 it is RefUnet's tail, conv_d0(d1) + x (:96-100).  x (B,Cin,h,wd) with batch
 * stride x_bs (0 = dense); w (1,Cin,3,3) and bias (1) as the module holds them; residual optional (B,1,h,wd); logits
 * (B,1,h,wd) REQUIRED (outconv1's are RefUnet's input); y optional (B,1,h*s,wd*s), batch stride y_bs (0 = dense).  The
 * up-sample is wsdl_bilinear_fwd's arithmetic (identical bits); sigmoid = 0 writes the up-sampled logits instead.  Each
 * pixel's dot product is summed in a fixed order: bitwise reproducible and independent of B.  Two launches. */
int wsdl_side_output(const float* x, long long x_bs, const float* w, const float* bias, const float* residual, int B,
                     int Cin, int h, int wd, int s, float* logits, float* y, long long y_bs, int sigmoid,
                     wsdl_stream_t stream);
/* RunInference.py's norm_pred (:36-40) per image, then (pred * 255).astype(np.uint8) (:77-83): out[b] = trunc(255 *
 * (d - min_b) / (max_b - min_b + 1e-8)) in float32 with contraction off, in ATen's order.  d (B,HW) fp32 with batch stride
 * d_bs (0 = dense; e.g. output #1 of a (B,1,H,W) tensor), out (B,HW) uint8.  One workgroup per image, two passes. */
int wsdl_saliency_u8(const float* d, long long d_bs, uint8_t* out, int B, int HW, wsdl_stream_t stream);

/* ---- fully-supervised baseline: segmentation metrics (csrc/seg_metrics.hip) ----
 * The per-batch counts of evaluate_model (reference FullySupervisedModel/SupervisedModel.py:44-83): preds = argmax over C
 * of logits (B,C,H,W) fp32 with torch.argmax's ties (the first maximum wins; NaN is the maximum, the first NaN wins),
 * compared with labels (B,H,W) int64.  counts: one row of 3C+1 int64 on the device,
 *   [0,C)   inter[c]  = #(pred = c and label = c)
 *   [C,2C)  npred[c]  = #(pred = c)
 *   [2C,3C) nlabel[c] = #(label = c)
 *   [3C]    correct   = #(pred = label)
 * A label outside [0,C) matches no class: it counts in npred of the predicted class and as a wrong pixel, as the
 * reference's boolean masks do.  union[c] = npred[c] + nlabel[c] - inter[c].  accumulate = 0 zeroes the row first (a
 * memset), 1 adds to it (one launch).  Integer counts only (block-local LDS histograms, one atomic per bin per block):
 * exact and independent of the schedule.  2 <= C <= 64 and B * HW < 2^32, other values are refused. */
int wsdl_seg_counts(const float* logits, const int64_t* labels, long long* counts, int B, int C, int HW, int accumulate,
                    wsdl_stream_t stream);

/* ---- Pillow's 8-bit resampling on the device (csrc/pil_resize.hip) ----
 * Image.resize(size, BILINEAR | BICUBIC) on 8-bit "RGB" / "L" images (box=None, reducing_gap=None), bit for bit: the
 * Resize((224, 224), BICUBIC) of the Oxford-IIIT Pet reader (reference TraditionalModel/ExtraUtilities.py:24-41) and the
 * Resize((256, 256)) (BILINEAR) of the stage-2 transforms (TraditionalModel/SegmentationDataset.py:19-28).  Pillow works in
 * integer fixed point (22 fractional bits, int32 sums, the horizontal pass first and rounded to uint8), so equality is exact.
 * The filter values are Pillow's Image.BILINEAR / Image.BICUBIC. */
#define WSDL_PIL_BILINEAR 2
#define WSDL_PIL_BICUBIC 3
/* HOST ONLY (no device is touched): the resampling table of one axis, computed in double the way Pillow computes it.
 * *ksize = (int)ceil(support * max(in / out, 1)) * 2 + 1 is always written.  bounds / kk may both be NULL (a size query);
 * else bounds[2 * i] = xmin, bounds[2 * i + 1] = xmax of output index i (out pairs) and kk[i * ksize + x] the int32
 * coefficient of source index xmin + x (zero for x >= xmax).  1 <= in, out <= 16384 and the two filters above; other
 * values are refused. */
int wsdl_pil_coeffs(int in, int out, int filter, int* ksize, int* bounds, int* kk);
/* One image of a batched resize: h x w x C interleaved uint8 (np.asarray of a PIL image) at src + src_off; htab / vtab:
 * offsets in int32 units into `tables` of the tables (w -> out_w) and (h -> out_h), each laid out as
 * [ksize | bounds (2 * out) | kk (out * ksize)]. */
typedef struct {
    long long src_off;
    int h, w;
    int htab, vtab;
} wsdl_pil_image_t;
/* N images of different sizes -> planar (N, C, out_h, out_w): uint8 in dst_u8 and / or float32 lut[c * 256 + u8] in dst_f32
 * (lut: C x 256 floats, e.g. ToTensor's u8 / 255 or ToTensor + Normalize; required with dst_f32).  src, images, tables and
 * the outputs are device memory.  One launch, no workspace, no atomics; results do not depend on N.  C in {1, 3} and
 * 1 <= out_h, out_w <= 16384, other values are refused; the images' own sides are checked by wsdl_pil_coeffs when their
 * tables are made. */
int wsdl_pil_resize_u8(const uint8_t* src, const wsdl_pil_image_t* images, const int* tables, int N, int C, int out_h,
                       int out_w, uint8_t* dst_u8, float* dst_f32, const float* lut, wsdl_stream_t stream);

/* ---- joint image / label augmentation of a training batch (csrc/augment.hip) ----
 * The reference has no counterpart: its pipelines resize and normalise only.  This is what the training loops need beyond
 * it, and it plugs into the device loaders that stand in for FullySupervisedModel/SupervisedModel.py:18-27
 * (PetDataset.DeviceLoader) and TraditionalModel/SegmentationDataset.py:19-28 (InMemoryPseudoDataset.batches): one launch
 * does their index gather, the uint8 -> float table and the label mapping, plus an affine warp and a gain / bias.
 *
 *   src        the image source, N x C x H x W dense: float32 (src_is_u8 = 0), or uint8 (src_is_u8 = 1) read through
 *              lut, C x 256 floats, value = lut[c * 256 + u8] (the table of wsdl_pil_resize_u8)
 *   src_label  N x H x W uint8; label_lut: 256 int64, raw byte -> class, NULL = identity
 *   idx        B int64: item b reads source row idx[b] (repeats and any order are legal; a row outside [0, N) reads
 *              nothing and yields an all-padding item)
 *   params     B x 8 float32: a00 a01 a02 a10 a11 a12 gain bias, the map from output to source coordinates
 *   images_out B x C x out_h x out_w float32, labels_out B x out_h x out_w int64
 * All of these are device memory.  Per output pixel (ox, oy), pixel i covering [i, i + 1):
 *   u = ox + 0.5f, v = oy + 0.5f
 *   xs = (a00 * u + a01 * v) + a02,  ys = (a10 * u + a11 * v) + a12
 *   fill = WSDL_AUGMENT_REFLECT:  P = 2 * W; q = floorf(xs / P); r = xs - P * q; if (r < 0) r += P; if (r >= W) r = P - r;
 *                                 xs = r  (and ys with H): the source mirrored about its borders, numpy's "symmetric"
 *   inside = fill == reflect, or (0 <= xs < W and 0 <= ys < H)
 *   label:  inside ? label_lut[src_label[min(floor(ys), H - 1)][min(floor(xs), W - 1)]] : pad_label
 *   image:  xc = xs - 0.5f, x0 = floor(xc), fx = xc - x0 (likewise y); the taps x0, x0 + 1, y0, y0 + 1 clamped to the
 *           source (replicate); top = v00 + fx * (v01 - v00); bot = v10 + fx * (v11 - v10); val = top + fy * (bot - top);
 *           inside ? gain * val + bias : pad_value
 * Every coordinate operation above is float32 and rounded on its own (no FMA contraction), so a float32 restatement selects
 * the same source pixels; validity is shared by image and label, so the padded regions coincide and padding never bleeds
 * into the image.  With fx = fy = 0, gain = 1, bias = 0 the output is the (finite) source value exactly: the identity
 * parameters 1 0 0 0 1 0 1 0 at out = source size reproduce the plain gather.  One launch, no workspace, no atomics; 64-bit
 * offsets throughout; results do not depend on B.  C in {1, 3}, 1 <= H, W, out_h, out_w <= 16384 and the two fills; other
 * values are refused on the host before any device is touched. */
#define WSDL_AUGMENT_IGNORE 0
#define WSDL_AUGMENT_REFLECT 1
int wsdl_augment_batch(const void* src, int src_is_u8, const float* lut, const uint8_t* src_label,
                       const long long* label_lut, const long long* idx, const float* params, int N, int C, int H, int W,
                       int B, int out_h, int out_w, int fill, float pad_value, long long pad_label, float* images_out,
                       long long* labels_out, wsdl_stream_t stream);

/* ---- losses --------------------------------------------------------------------------------- */
size_t wsdl_reduce_workspace(void);
/* ---- LossFunctions/Lovasz-Softmax_Loss.py (csrc/lovasz_seg.hip) ----
 * One segmented pipeline for the hinge and for every form of Lovasz-softmax.  A segment is an image (per_image) or the
 * batch, times a class: ONE device-wide stable radix sort (rocPRIM) of the order-preserving bits of the error - 32-bit keys
 * for one segment, 64-bit keys with the segment id above them otherwise -, ONE scan of the packed counts, one pass with the
 * Jaccard differences in fp32, the reference's arithmetic (a class list: one sort of all its entries; 'present' / 'all':
 * class after class).  Bitwise reproducible; ties are ranked by pixel index.  Refused on the host, before anything is
 * launched: 2^30 pixels or 2^32 sorted elements or more in all, a null pointer and, for the hinge and the class list, a
 * segment of 2^24 pixels or more.  ignore_label: pixels with that label take no part (pass a value no label has, e.g. -1,
 * for None).
 *
 * lovasz_softmax(probas, labels, classes='present' | 'all', per_image, ignore) - the optional loss of
 * train_segmentation_model (TraditionalModel/SegmentationModel.py:103-105; lovasz_grad :11-23, lovasz_softmax :146-161,
 * lovasz_softmax_flat :164-192, flatten_probas :195-211).  probas (B,C,H,W) class probabilities, labels int64 (B,H,W).
 * *loss = mean over the classes that occur (classes_all = 0, 'present') or over all C (classes_all = 1, 'all') of
 * <errors sorted descending, Jaccard-gradient of the sorted foreground>, of the batch or, per_image, its mean over the
 * images, each with its own classes (an image without a valid pixel is a zero term that counts); dprobas (optional,
 * (B,C,H,W)) = d loss / d probas (the Jaccard gradient is a constant of the sort order, as in the reference). */
size_t wsdl_lovasz_softmax_workspace(int B, int C, int H, int W, int per_image);
int wsdl_lovasz_softmax_fwd_bwd(const float* probas, const int64_t* labels, float* loss, float* dprobas, int B, int C,
                                int H, int W, int classes_all, int per_image, long long ignore_label, void* ws,
                                size_t ws_bytes, wsdl_stream_t stream);
/* lovasz_hinge(logits, labels, per_image=True, ignore=None) - LossFunctions/Lovasz-Softmax_Loss.py:71-119 (lovasz_hinge
 * :71-84, lovasz_hinge_flat :87-104, flatten_binary_scores :107-119; lovasz_grad :11-23).  logits (B,H,W) fp32
 * (channels = 1) or (B,2,H,W) (channels = 2: the binary logit is plane 1 - plane 0), labels int64 (B,H,W) in {0, 1,
 * ignore_label}.  e = 1 - logit * (2 label - 1); *loss = mean over the segments (per_image: the images; else the one
 * batch) of <relu(e) sorted descending, Jaccard gradient of the sorted labels>; an image without a valid pixel is a zero
 * term that counts in the mean.  dlogits (optional, the logits' shape) = d loss / d logits: -sign g_k / #segments where
 * e > 0, exactly 0 elsewhere and on ignored pixels; with two planes +d on plane 1 and -d on plane 0. */
size_t wsdl_lovasz_hinge_workspace(int B, int H, int W, int per_image);
int wsdl_lovasz_hinge_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B, int channels,
                              int H, int W, int per_image, long long ignore_label, void* ws, size_t ws_bytes,
                              wsdl_stream_t stream);
/* lovasz_softmax(probas, labels, classes=[...], per_image, ignore) - LossFunctions/Lovasz-Softmax_Loss.py:146-211
 * (lovasz_softmax :146-161, lovasz_softmax_flat :164-192, flatten_probas :195-211) for an explicit class list: classes is
 * a HOST array of n_classes (1..1024) channel numbers; every entry is a term whether or not the class occurs; *loss = mean
 * over the entries, per_image: the mean over the images of that (an image without a valid pixel is a zero term - the
 * reference returns an empty tensor there).  C = 1 (one sigmoid map) takes exactly one entry c and compares channel 0 with
 * labels == c.  dprobas optional, (B,C,H,W); channels that are not listed get zeros. */
size_t wsdl_lovasz_softmax_classes_workspace(int B, int C, int H, int W, int n_classes, int per_image);
int wsdl_lovasz_softmax_classes_fwd_bwd(const float* probas, const int64_t* labels, float* loss, float* dprobas, int B, int C,
                                        int H, int W, const int* classes, int n_classes, int per_image, long long ignore_label,
                                        void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* The counts of iou_binary / iou - LossFunctions/Lovasz-Softmax_Loss.py:26-65: preds, labels int64 (B,HW); per image
 * (per_image = 1; else one row for the batch) and class c < C, counts[(img * C + c) * 2 + 0] = #(label = c and pred = c),
 * [.. + 1] = #(label = c or (pred = c and label != ignore_label)); int64 on the device, overwritten.  The divisions, EMPTY,
 * the mean and the x 100 are the host's (Python floats in the reference). */
int wsdl_iou_counts(const int64_t* preds, const int64_t* labels, long long* counts, int B, int HW, int C, int per_image,
                    long long ignore_label, wsdl_stream_t stream);
/* binary_xloss / StableBCELoss - LossFunctions/Lovasz-Softmax_Loss.py:122-140: logits fp32 and EITHER labels int64 (t = the
 * label, pixels with label == ignore_label left out: binary_xloss) OR targets fp32 (every element counts: StableBCELoss), n
 * each; *loss = mean over those pixels of max(x,0) - x t + log(1 + exp(-|x|)) (NaN without one);
 * dlogits (optional) = its derivative, NOT yet divided by the count; *inv_count = 1 / count (0 without a valid pixel).
 * xloss :213-217 is wsdl_softmax_ce_fwd_bwd with ignore_index 255; isnan / mean :221-243 are host helpers.
 * ws: wsdl_reduce_workspace() bytes. */
int wsdl_binary_xloss_fwd_bwd(const float* logits, const int64_t* labels, const float* targets, float* loss, float* dlogits,
                              float* inv_count, long long n, long long ignore_label, void* ws, size_t ws_bytes,
                              wsdl_stream_t stream);

/* ---- dense-CRF refinement of pseudo masks (csrc/crf.hip) -------------------------------------------------------
 * apply_dense_crf(img_np, cam_np) of the notebook pipeline (TraditionalModel/AlternatingDirectionCutLoss.py:183-204, called
 * at :558 on the LayerCAM thresholded at :527-530): pydensecrf DenseCRF2D(W, H, 2) with
 *   unary      -log(clip(clip([1 - cam, cam], 1e-8, 1), 1e-5, 1))       (np.clip + unary_from_softmax),
 *   Gaussian   features (x/sxy, y/sxy), sxy = 1, PottsCompatibility(2)                     (addPairwiseGaussian defaults),
 *   bilateral  features (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb), sxy = 50, srgb = 5, Potts(10),
 *   both DIAG_KERNEL, NORMALIZE_SYMMETRIC, inference(5), argmax over the labels (ties -> label 0).
 * The filter is the permutohedral lattice (Adams et al. 2010) as densecrf builds it; the oracle is tests/crf_oracle.py
 * (parity with pydensecrf itself is not verified).  rgb: (B,H,W,3) uint8 (the notebook's
 * (img*255).astype(uint8)); cam (B,H,W) fp32 with values below cam_thresh set to 0 (pass -INFINITY for none), or an
 * explicit unary (B,2,H,W) fp32 instead (cam = NULL).  mask (B,H,W) uint8 {0,1}; q (optional, (B,2,H,W)) the final Q.
 * n_labels must be 2 (WSDL_EINVAL otherwise).  All images of the batch go through every launch: (lattice build + normaliser)
 * x 2 terms + n_iter x 2 x (splat + d+1 blurs + slice); no float atomics - bitwise reproducible and independent of B.
 * Coordinates of lattice keys are 16-bit fields: images up to ~4700 pixels on a side at sxy = 1 (WSDL_EINVAL beyond).
 * The workspace (wsdl_dense_crf_workspace) also serves the two diagnostic entry points below. */
size_t wsdl_dense_crf_workspace(int B, int H, int W, int n_labels);
int wsdl_dense_crf(const uint8_t* rgb, const float* cam, const float* unary, float cam_thresh, int B, int H, int W,
                   int n_labels, int n_iter, float gauss_sxy, float gauss_compat, float bil_sxy, float bil_srgb,
                   float bil_compat, uint8_t* mask, float* q, void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* (B,3,H,W) fp32 image in [0,1] -> (B,H,W,3) uint8 by truncating x*255 (the notebook's astype(np.uint8), :551-556),
 * clamped to [0, 255]. */
int wsdl_dense_crf_quantize(const float* img, uint8_t* out, int B, int H, int W, wsdl_stream_t stream);
/* Diagnostics of one feature set (bilateral = 0: Gaussian d = 2, 1: bilateral d = 5):
 * lattice: per (pixel, vertex) the d integer key coordinates (keys, (B*H*W, d+1, d) int32) and the barycentric weight
 * (bary, (B*H*W, d+1)); points (B) the number of lattice points of each image.
 * filter: out = K~ in = n * Lattice(n * in), n = 1/sqrt(Lattice(1) + 1e-20), on (B,2,H,W) fp32. */
int wsdl_dense_crf_lattice(const uint8_t* rgb, int B, int H, int W, int bilateral, float sxy, float srgb, int* keys,
                           float* bary, int* points, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_dense_crf_filter(const uint8_t* rgb, const float* in, float* out, int B, int H, int W, int n_labels, int bilateral,
                          float sxy, float srgb, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* nn.CrossEntropyLoss() on (B,C,H,W) logits and int64 (B,H,W) labels
 * (TraditionalModel/SegmentationModel.py:90,107; AlternatingDirectionCutLoss.py:789,699): mean over the pixels whose
 * label != ignore_index (PyTorch's default is -100; such pixels get zero loss and zero gradient).  Any other label
 * outside [0,C) - PyTorch raises - makes the loss NaN: a kernel cannot raise, and it must not train the pixel as a
 * real class.  dlogits (optional) = grad_scale * (softmax - onehot), NOT yet divided by the valid-pixel count:
 * *inv_count (device scalar, required with dlogits) receives 1/count and is applied together with the upstream
 * gradient (wsdl_scale_by_device_scalar). */
int wsdl_softmax_ce_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits,
                            float* inv_count, int B, int C, int H, int W, float grad_scale,
                            long long ignore_index, void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing) extended by a per-pixel weight: the same kernel
 * with its options switched on (wsdl_softmax_ce_fwd_bwd is this call with none of them).  For pixel i with label y,
 * softmax s, class weights w (class_weight, C floats, or null: all 1), pixel weight p (pixel_weight, B*H*W floats >= 0,
 * or null: all 1; p == 0 is an ignored pixel) and e = label_smoothing in [0, 1]:
 *     l_i = p_i * [ (1-e) w[y] (-log s[y]) + (e/C) sum_c w[c] (-log s[c]) ]        (0 where y == ignore_index)
 * reduction 0 (mean): *loss = sum_i l_i / sum_i p_i w[y_i] (PyTorch's denominator: the target classes only, also with
 * smoothing; 0/0 = NaN), *inv_count = 1 / that denominator; 1 (sum): *loss = sum_i l_i, *inv_count = 1; 2 (none): loss
 * points at B*H*W floats and receives l, inv_count is not written (may be null).  dlogits (optional) = grad_scale *
 * d l_i / d logits, still to be multiplied by inv_count x the upstream gradient (wsdl_scale_by_device_scalar) or, for
 * reduction 2, by the upstream gradient of each pixel (wsdl_scale_by_pixel).  A label outside [0,C) that is not
 * ignore_index: NaN loss (reduction 2: NaN at that pixel only).  Deterministic: fixed-order partial sums, no atomics. */
int wsdl_softmax_ce_ex_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits,
                               float* inv_count, int B, int C, int H, int W, float grad_scale,
                               long long ignore_index, const float* class_weight, const float* pixel_weight,
                               float label_smoothing, int reduction, void* ws, size_t ws_bytes,
                               wsdl_stream_t stream);
/* out[b,c,h,w] = dl[b,c,h,w] * g[b,h,w]: the backward of nn.CrossEntropyLoss(reduction='none') */
int wsdl_scale_by_pixel(const float* dl, const float* g, float* out, int B, int C, int H, int W,
                        wsdl_stream_t stream);
/* Pairwise-affinity loss over a reflect-padded window x window neighbourhood:
 *   apply_softmax=1, normalise=0, sigma_space<=0 : LocalNormalizedCutLoss.forward
 *                                  (TraditionalModel/AlternatingDirectionCutLoss.py:65-105)
 *   apply_softmax=0, normalise=1                 : ConstrainToBoundaryLossSingle.forward
 *                                  (TraditionalModel/AlternatingDirectionBoundaryLoss.py:12-70)
 * loss: 1 float (normalise=0) or B floats (normalise=1).  dpreds (optional) = d loss / d preds for
 * an upstream gradient of 1 (per image for normalise=1).
 * cache (optional): the image's colour affinities from wsdl_pairwise_cache (same B, H, W, window, sigma_color); the
 * kernel then reads them instead of evaluating 24 exponentials per pixel - refine_pseudo_mask evaluates the loss 10 x 5
 * times on one image (AlternatingDirectionCutLoss.py:736-757, :803-810).  Bit-identical results either way.
 * Accepted: window in {3, 5, 7}; H and W > window / 2 (one reflection, as F.pad); 1 <= C <= 32 and, at window 7,
 * C <= 27: the (3 + C) x (32 + 2R) x (8 + 2R) float tile of a workgroup must fit 64 KiB of LDS (R = window / 2; 60480
 * bytes at window 5 and C = 32, 63840 at window 7 and C = 27); 1 <= B <= 65535; sigma_color > 0; sigma_space <= 0 is "no
 * spatial term".  Anything else: WSDL_EINVAL with the cause in wsdl_last_error, nothing launched. */
int wsdl_pairwise_affinity_loss_fwd_bwd(const float* preds, const float* image, float* loss,
                                        float* dpreds, int B, int C, int H, int W, int window,
                                        float sigma_color, float sigma_space, int apply_softmax,
                                        int normalise, const float* cache, void* ws, size_t ws_bytes,
                                        wsdl_stream_t stream);
size_t wsdl_pairwise_workspace(int B, int H, int W);
/* exp(-|I_q - I_p|^2 / (2 sigma_color^2)) for the (window^2 - 1) / 2 "forward" offsets of every pixel (the affinity
 * is symmetric): cache[(window^2-1)/2][B][H][W] floats, wsdl_pairwise_cache_bytes of them. */
size_t wsdl_pairwise_cache_bytes(int B, int H, int W, int window);
int wsdl_pairwise_cache(const float* image, float* cache, int B, int H, int W, int window, float sigma_color,
                        wsdl_stream_t stream);
/* compute_affinities (TraditionalModel/AlternatingDirectionCutLoss.py:612-637): K=(w*w-1) maps,
 * out[(k*B + b)*H*W + p]. */
int wsdl_compute_affinities(const float* image, float* out, int B, int H, int W, int window,
                            float sigma_color, float sigma_space, wsdl_stream_t stream);

/* ---- LayerCAM epilogue (TraditionalModel/LayerCAM.py:52-76; variant 1 = notebook arithmetic,
 * AlternatingDirectionCutLoss.py:261-284) + threshold of PsuedoMasks.py:59-62 ------------------
 * act[l], grad[l]: (B,C[l],h[l],w[l]) device pointers, given as HOST arrays of n_layers entries.
 * cam: (B,outH,outW).  mask (optional, thresh >= 0): uint8 (cam >= thresh && cam > 0).
 * Every operation and the ORDER of the channel sum follow the reference's PyTorch-CPU path (ATen cascade_sum; bilinear
 * weights and blends as UpSampleKernel.cpp evaluates them): on identical act / grad the CAM and the mask are bit-identical
 * to the reference's for alpha in {1, 0.5, 2, 3} (csrc/layercam_optim.hip; option layercam_tail_mod). */
size_t wsdl_layercam_workspace(int n_layers, int B, const int* C, const int* h, const int* w);
int wsdl_layercam_epilogue(const float* const* act, const float* const* grad, const int* C,
                           const int* h, const int* w, int n_layers, int B, int outH, int outW,
                           float alpha, int variant, float* cam, float thresh, uint8_t* mask,
                           void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* The class-logit head of the LayerCAM pass in one call (TraditionalModel/LayerCAM.py:41-48 - `logits, _ = model(images)`,
 * `class_idx = argmax(logits)` when none is given, `logits.gather(1, class_idx).backward(ones)` - through
 * ClassificationModel.py:35-37, `fc(avgpool(f4).view(B, -1))`): pooled (B,C) = wsdl_global_avgpool_fwd of layer4's output,
 * weight (K,C), bias (K) or NULL, class_idx (B) int64 or NULL -> logits (B,K), cls (B) int32 (the class each image was
 * differentiated for; -1 and a NaN gradient for an index outside [0,K)), dx (B,C,HW) = weight[cls[b]][c] / HW: the gradient of
 * the chosen logit with respect to layer4's output (fc's backward followed by the average pool's, exactly: both are linear).
 * The parameters' own gradients (fc.weight.grad, fc.bias.grad - a side effect of the reference's backward nothing reads)
 * are not formed. */
int wsdl_class_logit_head(const float* pooled, const float* weight, const float* bias, const long long* class_idx,
                          float* logits, int* cls, float* dx, int B, int C, int K, int HW, wsdl_stream_t stream);

/* keep_largest (TraditionalModel/PsuedoMasks.py:15-21: skimage label + regionprops, the largest area wins, the first
 * label on ties, an empty mask stays empty) for n masks (n,h,w) of uint8 (non-zero = foreground) -> out (n,h,w) in {0,1};
 * 8-connectivity, labels in raster order of a component's first pixel as skimage numbers them.  One workgroup per mask,
 * labels in LDS up to 65535 pixels (224 x 224), in the workspace beyond.  out may alias mask.  Bit-exact. */
size_t wsdl_keep_largest_workspace(int n, int h, int w);
int wsdl_keep_largest(const uint8_t* mask, uint8_t* out, int n, int h, int w, void* ws, size_t ws_bytes,
                      wsdl_stream_t stream);

/* classic CAM normalisation (CAMGenerator.generate_all_cams, TraditionalModel/AlternatingDirectionCutLoss.py:343-372):
 * y = (relu(x) - min) / ((max - min) + 1e-8) per plane (min, max of relu(x)); the class-weighted channel sum itself is wsdl_conv2d_fwd with
 * fc.weight as a 1x1 kernel. */
int wsdl_plane_relu_minmax(const float* x, float* y, int planes, int hw, wsdl_stream_t stream);

/* ---- optimiser: torch.optim.Adam defaults (TraditionalModel/SegmentationModel.py:91,109-111) -
 * one launch over a flat parameter / gradient buffer; grad_scale folds the 1/world_size of DP.
 * step_dev (optional): the step number as a device int (bias corrections computed in the kernel) - for captured
 * (hipGraph) launches, where a host `step` would be frozen at capture time. */
int wsdl_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                   float beta2, float eps, int step, const int* step_dev, float grad_scale, wsdl_stream_t stream);
/* The same step with EVERY per-step quantity on the device: hyper_dev = {lr, beta1, beta2, eps, grad_scale} (five floats) and
 * the step number step_dev - a learning-rate schedule then changes five floats in device memory, not a kernel argument, so a
 * recorded launch plan (below) stays valid. */
int wsdl_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper_dev, const int* step_dev,
                       wsdl_stream_t stream);

/* ---- flat optimiser: SGD momentum / Adam + L2 / AdamW, global-norm clipping, non-finite skip (csrc/flat_optim.hip) -
 * Every per-step quantity is read from device memory (a recorded plan or a captured graph stays valid when one changes):
 * hyper_dev = WSDL_FLAT_HYPER floats {lr, beta1, beta2, eps, grad_scale, weight_decay, momentum, nesterov, max_norm,
 * skip_nonfinite} - the first five as wsdl_adam_step_dev reads them; stats_dev = WSDL_FLAT_STATS floats {total_norm,
 * clip_coef, apply, skipped_steps}.
 *
 * Gradient norm in two launches ordered by the stream (no atomics, no last-block counter: bit-reproducible).
 * wsdl_grad_sqnorm_partials: a fixed grid of wsdl_grad_norm_partials() workgroups of 256 threads, 16-byte loads, grid
 * stride; every element is squared and summed in double from the first product (1e18 does not overflow, 1e-30 does not
 * vanish); fixed order inside the workgroup -> one double per workgroup in `partials` (wsdl_grad_norm_workspace() bytes,
 * 16-byte aligned g). */
#define WSDL_FLAT_HYPER 10
#define WSDL_FLAT_STATS 4
#define WSDL_FLAT_ADAM_L2 0
#define WSDL_FLAT_ADAMW 1
#define WSDL_FLAT_SGD 2
int wsdl_grad_norm_partials(void);
size_t wsdl_grad_norm_workspace(void);
int wsdl_grad_sqnorm_partials(const float* g, size_t n, double* partials, wsdl_stream_t stream);
/* One workgroup sums n_partials doubles in fixed order and writes stats_dev: total_norm = |grad_scale| sqrt(sum);
 * clip_coef = min(1, max_norm / (total_norm + 1e-6)) when max_norm > 0, else 1 (torch.nn.utils.clip_grad_norm_);
 * apply = 0 when skip_nonfinite is set and the norm is inf / NaN, else 1.  A skipped step adds 1 to skipped_steps and takes
 * 1 from *step_dev (later bias corrections are those of a run that did not call step()).  The norm is judged AS THE FLOAT
 * that total_norm reports: a norm that is finite in double but above FLT_MAX (a few elements of 3e38) is inf there and is
 * skipped; clip_coef is taken from the double. */
int wsdl_grad_clip_finalize(const double* partials, int n_partials, const float* hyper_dev, int* step_dev, float* stats_dev,
                            wsdl_stream_t stream);
/* One launch over the flat buffers; g is multiplied by grad_scale * clip_coef first, then
 *   WSDL_FLAT_ADAM_L2: g += wd p; Adam                          (torch.optim.Adam(weight_decay=))
 *   WSDL_FLAT_ADAMW:   p *= 1 - lr wd; Adam                      (torch.optim.AdamW)
 *   WSDL_FLAT_SGD:     g += wd p; m = mu m + g; g = nesterov ? g + mu m : m; p -= lr g   (dampening 0, zero-initialised m;
 *                      mu = 0: m is neither read nor written and may be NULL; v may be NULL always).  The host cannot see
 *                      mu: with m == NULL the kernel runs SGD WITHOUT momentum whatever hyper_dev says - a caller whose
 *                      momentum may be non-zero passes m (optim.FlatSGD raises when momentum is set without a buffer).
 * decay_blocks (optional): one byte per 64 floats of the buffer, 1 = weight decay applies, 0 = it does not; NULL = everywhere.
 * stats_dev (optional): NULL = no clipping, no skip; apply == 0 leaves p, m, v untouched.  16-byte aligned buffers. */
int wsdl_flat_step_dev(int algo, float* p, const float* g, float* m, float* v, size_t n, const uint8_t* decay_blocks,
                       const float* hyper_dev, const int* step_dev, const float* stats_dev, wsdl_stream_t stream);

/* ---- EMA teacher: the average of the weights over training, and the teacher's label correction (csrc/ema.hip) -
 * The "mean teacher" copy (Tarvainen & Valpola, NeurIPS 2017) of the flat parameter buffer, as launches ordered behind the step
 * launch.  Per element, in double and rounded once:  e <- float( fma(a, double(p) - double(e), double(e)) ),  a = 1 - d,
 * d = decay, or with warm-up d = min(decay, float((1 + k) / (10 + k))) - the ratio formed in double and rounded to float32, so
 * that d is a float either way and a a dyadic number of at most 27 bits (a 53-bit 9 / (10 + k) puts exact results on float32
 * ties, which fused and unfused evaluations break differently) -, k = max(0, *step_dev - *start_dev - 1) = the updates already
 * applied: step_dev is the optimiser's device step number (a skipped step does not advance it), start_dev a device copy of it
 * taken when the average was attached or reset.  hyper_ema_dev = two floats {decay, warmup != 0} in device memory; a is formed
 * in double from the float decay.  a == 1 (decay 0) is a copy, e = p exactly.  stats_dev (optional) is the flat optimiser's:
 * apply == 0 returns at once, e untouched.  A NaN or inf in p propagates into e: skip_nonfinite is the guard, there is none here.
 * wsdl_flat_ema: one launch over n floats, float4 loads and stores, grid stride over a capped grid, a scalar tail of n & 3
 * elements; 16-byte aligned, non-overlapping buffers.  No atomics: bitwise reproducible.
 * wsdl_ema_table: one launch for many small tensors (BatchNorm running statistics): table_dev = `count` wsdl_ema_entry in device
 * memory; workgroup (x, y) handles the chunks y, y + 4, ... of 1024 floats of the tensors x, x + gridDim.x, ...; mode 0 = the
 * formula above, mode 1 = dst = src (hyper_ema_dev, step_dev, start_dev may then be NULL).  4-byte aligned pointers: a tensor
 * whose two pointers are not both 16-byte aligned takes a scalar path.  The same skip test.  Tensors must not overlap. */
typedef struct {
    float* dst;
    const float* src;
    long long numel;
} wsdl_ema_entry;
int wsdl_flat_ema(float* e, const float* p, size_t n, const float* hyper_ema_dev, const int* step_dev, const int* start_dev,
                  const float* stats_dev, wsdl_stream_t stream);
int wsdl_ema_table(const wsdl_ema_entry* table_dev, int count, const float* hyper_ema_dev, const int* step_dev, const int* start_dev,
                   const float* stats_dev, int mode, wsdl_stream_t stream);
/* Label correction from teacher logits (B,C,H,W) float32, C <= WSDL_TEACHER_MAX_CLASSES, and the current labels (B,H,W) int64, one
 * pass: t = the first class of largest logit, p = float(1 / sum_c exp(double(l_c) - double(l_t))) (the softmax maximum); a pixel
 * with any non-finite logit has p = 0 and is never confident; a pixel is confident iff p >= *tau_dev (one float in device
 * memory).  y == ignore_index: y' = y, conf = 0.  Otherwise conf = p and, where the pixel is confident and t != y, y' = t (mode 0,
 * "replace") or y' = ignore_index (mode 1, "ignore"); else y' = y.  out_conf (B,H,W) float32 and counts may be NULL; counts[0..2]
 * += (pixels with y' == y that were not ignored on input, pixels with y' != y, pixels ignored on input) - integer atomics, one
 * per counter and workgroup: exact and order-independent.  Four pixels per lane where H W % 4 == 0; the channels of C = 2 and 3
 * are held in registers, any other C reads its pixel's channels twice (no per-lane array: no scratch).  No host read, every
 * parameter by value: a launch plan can hold the call. */
#define WSDL_TEACHER_MAX_CLASSES 64
int wsdl_teacher_targets(const float* logits, const long long* labels, int B, int C, int H, int W, const float* tau_dev, int mode,
                         long long ignore_index, long long* out_labels, float* out_conf, long long* counts, wsdl_stream_t stream);

/* ---- view consistency: warps of score / label maps and the consistency loss (csrc/consistency.hip) ----
 * The reference has no counterpart.  A prediction made on one view of an image is compared with the prediction on another
 * view: warp one onto the other by the augmentation's affine map, compare two per-pixel class distributions where the warp is
 * valid and the teacher is confident, differentiate.
 *
 * THE COORDINATE RULE is the one of wsdl_augment_batch above, word for word (csrc/warp_coords.h): params is B x 8 float32,
 * a00 a01 a02 a10 a11 a12 gain bias, mapping output pixel (ox, oy) to the source point xs, ys with u = ox + 0.5f, every
 * operation float32 and rounded on its own; both fills; bilinear taps x0, x0 + 1, y0, y0 + 1 clamped (replicate), fractions
 * fx, fy; the nearest tap min(floor(xs), W - 1).  One rule is added: a NON-FINITE xs or ys (after the reflection, which keeps a
 * non-finite value non-finite) is "not inside" under both fills.  The value rule is top = v00 + fx * (v01 - v00),
 * bot = v10 + fx * (v11 - v10), val = top + fy * (bot - top), float32, unfused - where a fraction is 0 its lerp is skipped
 * and the first tap taken as it is, so with fx = fy = 0 the value is v00 bit for bit, +-inf included, whatever the unused taps hold.
 *
 * wsdl_warp_scores_fwd: src (B,C,h,w) float32, 1 <= C <= WSDL_CONSISTENCY_MAX_CLASSES -> out (B,C,out_h,out_w):
 * inside ? (photometric ? gain * val + bias : val) : pad_value; valid (B,out_h,out_w) uint8, may be NULL, receives `inside`.
 * wsdl_warp_labels: src (B,h,w) int64 -> out (B,out_h,out_w): inside ? src[nearest tap] : pad_label.
 * Both: one launch, no atomics, no workspace, 64-bit offsets, results independent of B; sides 1..16384.
 *
 * wsdl_warp_scores_bwd: the adjoint of wsdl_warp_scores_fwd with respect to src for fill = ignore: dsrc (B,C,h,w) =
 * sum over the inside output pixels of (weight of the tap (j,i)) * dy, the weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy,
 * fx fy formed in double from the forward's float32 fx, fy (taps that the clamp merges add up; times gain with photometric).
 * A gather - per source pixel the candidates are the output pixels in the bounding box of the inverse image (in double) of
 * [i - 0.5, i + 1.5] x [j - 0.5, j + 1.5] clipped to the image, widened by 2 pixels plus the forward's float32 rounding
 * carried through the inverse; each candidate recomputes the forward's taps; the sum runs in double in raster order and is
 * rounded once.  No atomics: bitwise reproducible.  A row with a non-finite coefficient has no inside pixel and gives zeros at
 * once; a finite singular row (or one whose inverse overflows) takes the whole output as its box, so the result never depends
 * on the magnification - only the time does: small boxes for magnifications in [1/4, 4], (h w) x (out_h out_w) tap evaluations
 * per chunk of 8 channels for the whole-output box (2^36 at 512 x 512 on both sides: a degenerate view, not a training case).
 * Source pixels
 * nothing taps receive exact zeros.  fill = reflect is refused: its adjoint is not built.
 *
 * wsdl_consistency_fwd_bwd: student (B,C,H,W) logits z; teacher (B,C,ht,wt), logits or probabilities (teacher_is); params
 * (B,8) the map from the STUDENT's pixel grid to the teacher's - the teacher is sampled at every student pixel by the rule
 * above (the float32 value wsdl_warp_scores_fwd would write, bit for bit; never materialised) - or NULL: same size, direct
 * read, no interpolation.  knobs: three floats in device memory, tau lam T.  Per pixel, in double:
 *   q = softmax(t / T) for logits; q = t / sum t for probabilities (T is not used);  s = softmax(z);  conf = max q
 *   counted = warp inside and every teacher value t_c and student logit finite (probabilities: and t_c >= 0, sum t > 0)
 *             and conf >= tau;      w = counted ? pixel_weight (B,H,W; NULL: 1) : 0
 *   kl:   l = sum_c q_c (log q_c - log s_c)                 dl/dz = s - q
 *   mse:  l = (1/C) sum_c (s_c - q_c)^2                     dl/dz_k = (2/C) s_k ((s_k - q_k) - sum_c s_c (s_c - q_c))
 *   hard: target = the first class of largest t, l = -log s_target   dl/dz = s - onehot(target)
 * loss = lam / N * sum_p w_p l_p, N = B H W (WSDL_CONSISTENCY_ALL) or sum_p w_p (WSDL_CONSISTENCY_COUNTED); dlogits (may be
 * NULL) receives the gradient of that loss, lam / N included, rounded once; with no counted pixel the loss is 0 and the
 * gradient exact zeros.  counts (2 int64, may be NULL) = {pixels inside, pixels counted}; weight_out (B,H,W) float32 = w;
 * target_out (B,H,W) int64 = the hard target at counted pixels, -100 elsewhere (both may be NULL).  A "finite teacher value"
 * is the interpolated one: a tap that the zero-fraction rule leaves unused may hold anything.
 * normalize = all: one fused pass and a one-workgroup finalize; normalize = counted with dlogits: a sums pass, the finalize,
 * a gradient pass.  Double partials per workgroup added in fixed order, no atomics: two calls give the same bits.  No host
 * read, every parameter by value or in device memory: a launch plan can hold the call.  C = 2 and 3 are held in registers,
 * any other C re-reads its pixel's values per pass (no per-lane array: no scratch).  ws: wsdl_consistency_workspace() bytes. */
#define WSDL_CONSISTENCY_MAX_CLASSES 64
#define WSDL_CONSISTENCY_KL 0
#define WSDL_CONSISTENCY_MSE 1
#define WSDL_CONSISTENCY_HARD 2
#define WSDL_CONSISTENCY_LOGITS 0
#define WSDL_CONSISTENCY_PROBS 1
#define WSDL_CONSISTENCY_ALL 0
#define WSDL_CONSISTENCY_COUNTED 1
int wsdl_warp_scores_fwd(const float* src, const float* params, int B, int C, int h, int w, int out_h, int out_w, int fill,
                         float pad_value, int photometric, float* out, uint8_t* valid, wsdl_stream_t stream);
int wsdl_warp_labels(const int64_t* src, const float* params, int B, int h, int w, int out_h, int out_w, int fill,
                     long long pad_label, int64_t* out, wsdl_stream_t stream);
int wsdl_warp_scores_bwd(const float* dy, const float* params, int B, int C, int h, int w, int out_h, int out_w, int fill,
                         int photometric, float* dsrc, wsdl_stream_t stream);
size_t wsdl_consistency_workspace(void);
int wsdl_consistency_fwd_bwd(const float* student, const float* teacher, const float* params, const float* pixel_weight,
                             const float* knobs, int B, int C, int H, int W, int ht, int wt, int kind, int teacher_is,
                             int normalize, int fill, float* loss, float* dlogits, long long* counts, float* weight_out,
                             long long* target_out, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* ---- batch mixing: CutMix / ClassMix / copy-paste as a selection (csrc/mix.hip) ----
 * The reference has no such step.  A batch has B items with planes of H x W (sides 1..16384).  partner (B) int32: item b is mixed
 * with item partner[b]; a value outside [0, B) leaves item b UNMIXED (its mask is 0 everywhere) - the value is tested before it
 * indexes anything; self-partners and duplicates are legal.  The mask M[b,y,x] in {0,1}, 1 = "take the partner's pixel":
 *   WSDL_MIX_BOX    boxes (B,R,4) int32, 1 <= R <= WSDL_MIX_MAX_BOXES, rows (y0, x0, y1, x1) half-open in pixels: M = 1 inside the
 *                   union of the R boxes; y1 <= y0 or x1 <= x0 contributes nothing; coordinates outside the image clip implicitly.
 *   WSDL_MIX_CLASS  M = 1 iff class_labels[partner[b],y,x] (int64) is a class of the 64-bit set sel[partner[b]]; a label outside
 *                   [0, 64) is never selected, and wsdl_mix_class_select sets no bit from C on, so neither is one outside [0, C).
 *   WSDL_MIX_MASK   mask (B,H,W) uint8: M = mask[b] != 0.
 * invert = 1 flips M for mixed items only.
 *
 * wsdl_mix_class_select: the ClassMix choice on the device, C <= WSDL_MIX_MAX_CLASSES.  Item i uses seeds[i] (int64) for its own
 * label map: present_i = the classes c < C with bit c of `candidates` set and some pixel class_labels[i] == c; n = |present_i|,
 * k = ceil(n / 2); key(c) = fmix(uint64(seeds[i]) + (c + 1) * 0x9E3779B97F4A7C15) modulo 2^64, fmix the splitmix64 finaliser
 * (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31); sel_i = the k present classes of
 * smallest (key, c), as a bit set; n = 0 gives the empty set.  present and sel (B) int64 receive the two sets.  A memset of
 * `present`, a presence launch (one 64-bit integer atomic OR per workgroup) and a one-wave-per-image selection launch.
 *
 * wsdl_mix_apply: for each of the n_tensors <= WSDL_MIX_MAX_TENSORS tensors (B, channels, H, W) of 4- or 8-byte elements,
 * dst[b,c,y,x] = M[b,y,x] ? src[partner[b],c,y,x] : src[b,c,y,x] - ONE launch for all of them, the mask evaluated once per pixel.
 * The outputs are bit copies (values move as integer words); inputs are never modified.  mask_out (B,H,W) uint8 and count_out (B)
 * int64 may be NULL: M itself, and the number of pixels with M = 1 (zeroed by a memset in front of the launch, then one integer
 * atomic per workgroup: exact, order-independent).  An output that overlaps an input or another output in memory is refused
 * (item b reads item partner[b]: in-place use is a race).  Four pixels per lane with 16-byte accesses where W % 4 == 0 and
 * every base is 16-byte aligned (mask, mask_out: 4-byte), one pixel per lane otherwise.  No host read, every parameter by value
 * or in device memory: a launch plan can hold both calls; two calls give the same bits. */
#define WSDL_MIX_MAX_CLASSES 64
#define WSDL_MIX_MAX_BOXES 8
#define WSDL_MIX_MAX_TENSORS 4
#define WSDL_MIX_BOX 0
#define WSDL_MIX_CLASS 1
#define WSDL_MIX_MASK 2
typedef struct wsdl_mix_tensor {
    const void* src;
    void* dst;
    int channels;
    int elem_bytes;
} wsdl_mix_tensor;
int wsdl_mix_class_select(const int64_t* class_labels, const int64_t* seeds, int B, int C, int H, int W, unsigned long long candidates,
                          int64_t* present, int64_t* sel, wsdl_stream_t stream);
int wsdl_mix_apply(const wsdl_mix_tensor* tensors, int n_tensors, const int32_t* partner, int kind, const int32_t* boxes, int R,
                   const int64_t* class_labels, const int64_t* sel, const uint8_t* mask, int invert, int B, int H, int W,
                   uint8_t* mask_out, int64_t* count_out, wsdl_stream_t stream);

/* ---- score histograms: grouped histograms with exact counts, threshold sweeps, Otsu, calibration (csrc/score_hist.hip) ----
 * The reference has no such step: its thresholds are constants.  A TABLE has G groups x (nb + 3) slots over nb + 1 edges (float32,
 * strictly ascending, finite, in device memory; edges_host is the same nb + 1 values in host memory, which the entry point checks -
 * nothing is read back from the device).  The slot of a value v is defined by comparisons against the edges alone:
 *   slot 0: v < edges[0];  slot 1 + k: edges[k] <= v < edges[k + 1];  slot nb + 1: v >= edges[nb] (+inf included);  slot nb + 2: NaN;
 *   -0.0 compares as 0.  For equally spaced edges the kernel guesses the slot arithmetically and then walks the guess to the slot the
 *   comparisons define; other edges take a binary search over their copy in LDS.
 * Limits: nb <= WSDL_HIST_MAX_BINS, G <= WSDL_HIST_MAX_GROUPS, G (nb + 3) <= WSDL_HIST_MAX_SLOTS, B <= 65535, a segment has fewer
 * than 2^31 pixels.
 *
 * wsdl_score_hist: scores (B,HW) float32, groups (B,HW) int64 or NULL (all group 0); a pixel whose group is outside [0, G) is not
 * counted.  counts (S,G,nb+3) int64 with S = B (per_image = 1) or 1: zeroed by a memset in front of the launch, then counts[s,g,slot]
 * = the number of pixels.  sums (same shape, may be NULL): the sum of (long long)(v * 16777216.0f) - an exact product, a truncating
 * conversion - over the pixels of the slots 1 .. nb, 0 elsewhere; with sums every edge must lie in [-128, 128].  One launch, grid
 * (chunks, images) of about 1024 workgroups: the table is privatised in LDS (32-bit counters, 64-bit sums; one copy per wave up to
 * 1040 slots, else one per workgroup), the per-pixel add is aggregated over the lanes of a wave that share a slot, and a workgroup
 * flushes its non-zero slots with 64-bit integer atomics.  Four pixels per lane with 16-byte loads where HW % 4 == 0 and scores and
 * groups are 16-byte aligned, else one.  An output that overlaps an input or the other output is refused.
 *
 * wsdl_confidence_hist: logits (B,C,H,W) float32, C <= WSDL_CONFIDENCE_MAX_CLASSES, labels (B,H,W) int64.  Per pixel pred = the
 * first class of largest logit and conf = float(1 / sum_c exp(double(l_c) - double(l_pred))), NaN where a logit is not finite;
 * a pixel with label != ignore_index is counted as wsdl_score_hist counts the value conf in group (pred == label) of a table with
 * G = 2 (sums as there).  conf_out (B,H,W) float32 and pred_out (B,H,W) int64 may be NULL; they are written at every pixel.
 *
 * wsdl_hist_curves: counts (S,2,nb+3), group 1 the positives -> curves (S,nb+1,4) int64 = TP FP FN TN of the prediction
 * v >= edges[k], k = 0 .. nb: the slots k + 1 .. nb + 1 are predicted positive, slot 0 and the NaN slot never.  One workgroup per
 * segment, suffix sums.
 *
 * wsdl_otsu: per segment over h_i = the sum over the groups of group_mask of counts[s,g,1+i], i = 0 .. nb - 1; N = sum h_i,
 * S = sum i h_i; for k = 0 .. nb - 2: w0 = sum_{i<=k} h_i, w1 = N - w0, s0 = sum_{i<=k} i h_i, s1 = S - s0, D = s0 w1 - s1 w0 (int64),
 * q(k) = (double(D) * double(D)) / double(w0 w1) where w0 w1 > 0.  k_out = the first maximum of q, threshold_out = edges[k + 1],
 * q_out = q(k); with fewer than two occupied bins k_out = -1, threshold_out = fallback, q_out = 0.  segment_pixels = the largest
 * N the caller vouches for (0: no claim), refused above 2^21, which keeps D below 2^53; a segment that holds more all the same gets
 * k_out = -2 and NaN.  One workgroup per segment.
 *
 * wsdl_threshold_images: mask[b,p] (uint8) = scores[b,p] >= thresh[b] && (!positive_only || scores[b,p] > 0); thresh (B) float32 in
 * device memory (NaN: an empty mask).  count (B) int64, may be NULL: the number of set pixels, zeroed by a memset in front of the
 * launch, one integer atomic per workgroup.
 *
 * All five: integer atomics only, so two calls give the same bits; no host read, every parameter by value or in device memory: a
 * launch plan can hold the calls. */
#define WSDL_HIST_MAX_BINS 1024
#define WSDL_HIST_MAX_GROUPS 32
#define WSDL_HIST_MAX_SLOTS 4096
#define WSDL_CONFIDENCE_MAX_CLASSES 64
int wsdl_score_hist(const float* scores, const int64_t* groups, const float* edges, const float* edges_host, int B, long long HW, int G,
                    int nb, int per_image, int64_t* counts, int64_t* sums, wsdl_stream_t stream);
int wsdl_confidence_hist(const float* logits, const int64_t* labels, const float* edges, const float* edges_host, int B, int C, int H, int W,
                         long long ignore_index, int nb, int per_image, int64_t* counts, int64_t* sums, float* conf_out, int64_t* pred_out,
                         wsdl_stream_t stream);
int wsdl_hist_curves(const int64_t* counts, int S, int nb, int64_t* curves, wsdl_stream_t stream);
int wsdl_otsu(const int64_t* counts, const float* edges, int S, int G, int nb, unsigned group_mask, float fallback, long long segment_pixels,
              int32_t* k_out, float* threshold_out, double* q_out, wsdl_stream_t stream);
int wsdl_threshold_images(const float* scores, const float* thresh, int B, long long HW, int positive_only, uint8_t* mask, int64_t* count,
                          wsdl_stream_t stream);

/* ---- pixel mining: selecting pixels by their loss without a host read (csrc/pixel_mining.hip) -
 * wsdl_kth_value: x holds `segments` runs of n_per_segment floats.  The candidates of segment s are the x[s*n + i] that are
 * not NaN and, when `valid` (one byte per element) is given, have valid[s*n + i] != 0; n_valid[s] receives their number n.
 * The rank is computed ON THE DEVICE, in double: k = min(n, k_abs + floor(k_frac * n)); value[s] = the k-th largest
 * candidate (largest != 0) or the k-th smallest - an element of x, bit for bit (-0.0 and +0.0 are different keys that
 * compare equal: either may come back).  k == 0 (n == 0 included): +inf for largest, -inf for smallest, so that a
 * ">= value" / "<= value" test keeps nothing.  Any finite float, denormals and +-inf are ordered by the usual monotone
 * 32-bit key.
 * Most-significant-digit radix select, 4 passes of 8 bits, each pass one launch on `stream` (plus the memset of the
 * workspace and a one-workgroup launch per segment that writes the results): workgroups count their digit in LDS -
 * privatised per wave, equal digits of a wave aggregated before the atomic - and merge with integer atomics into the
 * segment's histogram; every workgroup of the next pass finds the chosen bin for itself.  Nothing waits for another
 * workgroup, no float atomics: the result does not depend on the arrival order (bitwise reproducible).
 * ws: wsdl_kth_workspace(segments) bytes, 4-byte aligned.  1 <= n_per_segment < 2^31, 1 <= segments <= 65535,
 * k_abs >= 0, 0 <= k_frac <= 1. */
#define WSDL_MINING_HARD 0
#define WSDL_MINING_TRIM 1
size_t wsdl_kth_workspace(int segments);
int wsdl_kth_value(const float* x, const uint8_t* valid, long long n_per_segment, int segments, int largest, long long k_abs,
                   double k_frac, float* value, long long* n_valid, void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* valid_out[i] = 1 where labels[i] != ignore_index and (pixel_weight == NULL or pixel_weight[i] != 0), else 0: the pixels
 * wsdl_softmax_ce_ex_fwd_bwd does not ignore. */
int wsdl_mining_valid(const int64_t* labels, long long ignore_index, const float* pixel_weight, uint8_t* valid_out, long long n,
                      wsdl_stream_t stream);
/* The selection as a pixel weight for wsdl_softmax_ce_ex_fwd_bwd: weight_out[i] = pixel_weight[i] (or 1) where pixel i of
 * segment s is valid and selected, else 0.  WSDL_MINING_HARD selects nll >= min(tau[s], tau_cap) (tau: the k-th largest
 * loss, tau_cap = -log(thresh) or +inf: online hard example mining, at least k pixels), WSDL_MINING_TRIM selects
 * nll <= tau[s].  Ties at the threshold are all selected.  A valid pixel whose nll is NaN (a label outside [0,C)) keeps
 * its weight, so that the cross entropy is poisoned as it is without mining.  kept[s] = the number of selected pixels
 * (one integer per workgroup in ws, summed in fixed order by a second launch; no atomics).
 * ws: wsdl_mining_weights_workspace(segments) bytes, 4-byte aligned. */
size_t wsdl_mining_weights_workspace(int segments);
int wsdl_mining_weights(const float* nll, const uint8_t* valid, const float* pixel_weight, const float* tau, float tau_cap,
                        int mode, long long n_per_segment, int segments, float* weight_out, long long* kept, void* ws,
                        size_t ws_bytes, wsdl_stream_t stream);
/* out[i] = dl[i] * s[0] with a zero staying zero (wsdl_scale_by_device_scalar otherwise, same bits): when nothing is
 * selected the mean's denominator is 0 and s = inf - the gradient is then 0 everywhere, as torch's over ignored pixels. */
int wsdl_mining_scale_grad(const float* dl, const float* s, float* out, size_t n, wsdl_stream_t stream);

/* ---- PAMR: pixel-adaptive mask refinement (Araslanov & Roth, CVPR 2020; csrc/pamr.hip) - the reference has no such step -
 * A parameter-free local propagation of a score map m (B,C,H,W) whose weights come from the local contrast of an image
 * x (B,K,H,W) on the same H x W.  Neighbourhood: P = 8 n_dil pixels - for each dilation d, in the order given, the offsets
 * (dy d, dx d), dy, dx in {-1,0,1} in raster order without the centre; borders are replicated, q_j = (clamp(y + oy_j, 0, H-1),
 * clamp(x + ox_j, 0, W-1)), every coordinate on its own (below a dilation both borders clamp).
 *   sigma_k(p) = unbiased (n-1) deviation of the 9 n_dil samples x_k(q): 8 neighbours and the centre per dilation (the
 *                centre counts n_dil times); from the mean, sums in double - a flat neighbourhood gives exactly 0
 *   a(p,j)     = mean_k -|x_k(p) - x_k(q_j)| / (1e-8 + 0.1 sigma_k(p))
 *   w(p,.)     = softmax_j a(p,.)                                   (flat neighbourhood: exactly 1/P)
 *   one iteration: m'_c(p) = sum_j w(p,j) m_c(q_j)
 * The result does not depend on a per-channel gain or offset of the image (up to the 1e-8).  fp32 planes, dense NCHW.
 * 1 <= K <= 4, 1 <= C <= 32, 1 <= n_dil <= 8, 1 <= d <= 64, H W <= 2^28.  No atomics, no sum across threads: bitwise
 * reproducible.  Every launch copies the dilations by value, so a launch plan may hold the calls.
 * wsdl_pamr_affinity: weights (B,P,H,W), plane j = neighbour j (W-contiguous: the propagation reads them coalesced).
 * wsdl_pamr_propagate: n_iter iterations (one launch each per 4 score channels) from mask_in to mask_out, ping-pong
 *   between two buffers carved from ws (wsdl_pamr_workspace bytes, 16-byte aligned; not needed for n_iter < 2); the result
 *   lands in mask_out for every n_iter, n_iter = 0 copies; mask_in is never written; mask_in and mask_out must not overlap.
 * wsdl_pamr_workspace: 0 for a geometry outside the limits above (host-side check, no device touched).
 * wsdl_pamr_labels: labels_out (B,H,W) int64 - C >= 2: the index of the first maximum over the channels, ignore_index
 *   where that maximum is < min_conf; C == 1: 1 where m >= thresh, else 0 (min_conf is not used). */
size_t wsdl_pamr_workspace(int B, int C, int H, int W, int n_dil);
int wsdl_pamr_affinity(const float* image, int B, int K, int H, int W, const int* dilations, int n_dil, float* weights,
                       wsdl_stream_t stream);
int wsdl_pamr_propagate(const float* weights, const float* mask_in, float* mask_out, int B, int C, int H, int W,
                        const int* dilations, int n_dil, int n_iter, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_pamr_labels(const float* mask, int B, int C, int H, int W, float thresh, float min_conf, long long ignore_index,
                     long long* labels_out, wsdl_stream_t stream);

/* ---- distance transforms, Boundary IoU counts, boundary confidence (csrc/edt.hip) - the reference has no such step -
 * wsdl_edt: the exact squared distance transform of labels (B,H,W) int64.  A pixel p is IN if labels[p] == value and OUT
 * otherwise (void / ignore labels included).  Two int32 planes (B,H,W):
 *   d2_out[p] = min over the OUT pixels q of dist2(p,q)     (0 where p is OUT)
 *   d2_in[p]  = min over the IN pixels q of dist2(p,q)      (0 where p is IN)
 * Either pointer may be null: that plane is not computed (both null: nothing is launched).
 *   metric 0  Euclidean: dist2 = dy^2 + dx^2
 *   metric 1  Chebyshev: dist2 = max(|dy|,|dx|)^2 - what iterated 3 x 3 erosion measures (Boundary IoU, Cheng et al., CVPR 2021)
 *   border 0  only pixels of the image count
 *   border 1  everything outside the image is an OUT pixel for d2_out (a pixel in column x is at distance x + 1 from the
 *             outside); d2_in is the same for both values
 * Where no site exists - an all-IN image with border 0, d2_in of an image without an IN pixel - the value is the sentinel
 * WSDL_EDT_FAR.  1 <= H, W <= 8192 and B H W < 2^31: every true squared distance is then below 2^28 and cannot collide with
 * the sentinel, and no intermediate square leaves int32.  Other values are refused (WSDL_EINVAL) before any launch.
 * Integer arithmetic only, no atomics: exact, bitwise reproducible, independent of the schedule.  Two launches (columns,
 * rows); the planes themselves hold the intermediate; every parameter travels by value, so a launch plan may hold the call.
 * wsdl_band_counts: per image b over its HW pixels, with band X = (0 < d2_X <= limit2): counts[b*2+0] = #(band A and band B),
 *   counts[b*2+1] = #(band A or band B); int64 (B,2) on the device, overwritten (a memset and one launch).  With A, B the
 *   d2_out planes of a prediction and a ground truth (metric 1, border 1, limit2 = width^2) these are the intersection and
 *   union of Boundary IoU.  0 <= limit2 < WSDL_EDT_FAR, so the sentinel is in no band.  Block-local integer counts, one
 *   atomic per counter and block: exact whatever the schedule.
 * wsdl_boundary_confidence: w[p] = floor + (1 - floor) (1 - exp(-d2 / (2 sigma^2))) with d2 = d2_out[p] + d2_in[p] (one of
 *   the two is 0), fp32, n pixels; w = 1 where either plane holds the sentinel (an image without a boundary).
 *   0 <= floor <= 1, sigma > 0 and finite, 1 <= n < 2^31. */
#define WSDL_EDT_FAR (1 << 30)
int wsdl_edt(const int64_t* labels, long long value, int B, int H, int W, int metric, int border, int* d2_out, int* d2_in,
             wsdl_stream_t stream);
int wsdl_band_counts(const int* d2_a, const int* d2_b, int limit2, int B, int HW, long long* counts, wsdl_stream_t stream);
int wsdl_boundary_confidence(const int* d2_out, const int* d2_in, float sigma, float floor, float* w_out, size_t n,
                             wsdl_stream_t stream);

/* ---- signed-distance boundary loss, surface distances (csrc/boundary_loss.hip) - the reference has no counterpart: its
 * losses act on regions and pixels (cross entropy, Lovasz, the NCut and boundary-constraint terms) and its evaluation
 * reports region IoU and pixel accuracy.  Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019.
 * wsdl_signed_distance: no counterpart in the reference; the paper's one_hot2dist.  From the two Euclidean planes of wsdl_edt
 *   (border 0) of one class, per pixel: phi = +sqrt(d2_in) on OUT pixels (d2_out == 0), phi = -(sqrt(d2_out) - 1) on IN
 *   pixels - the published distance(negmask) * negmask - (distance(posmask) - 1) * posmask - and phi = 0 where either plane
 *   holds WSDL_EDT_FAR (the class is absent from the image or fills it: the whole image is 0).  The root is taken in double
 *   and rounded once.  phi[b * phi_batch_stride + p], p < HW; a stride of 0 means HW, K HW writes one plane of a (B,K,H,W) map.
 * wsdl_boundary_loss_fwd_bwd: no counterpart in the reference; the paper's SurfaceLoss, mean(softmax(logits)_c * phi_c), fused
 *   with its gradient.  logits (B,C,H,W) fp32, phi (B,K,H,W) fp32, class_list K distinct ints in [0, C) on the HOST (copied
 *   into the launch by value; 1 <= K <= 32): plane k of phi belongs to class class_list[k].  labels (B,H,W) int64 or null:
 *   a pixel is valid when labels[p] != ignore_index, every pixel without labels; N = #valid pixels.  With s = softmax over C
 *   and Phi_c = phi plane of class c, 0 for a class outside the list:
 *     loss = scale / (K N) * sum over valid p and c of s_c(p) Phi_c(p)
 *     dlogits[b,c,p] = s_c (Phi_c - sum_j s_j Phi_j), UN-normalised, 0 at invalid pixels (may be null)
 *     inv = scale / (K N)   (the factor the gradient still lacks; required with dlogits)
 *   scale = *scale_dev (a device float) or 1 when scale_dev is null.  N == 0: loss = 0 and inv = 0 - the term is an additive
 *   regulariser, a batch without a valid pixel adds nothing instead of NaN.  The softmax and the products are evaluated in
 *   double and each output is rounded once.  ws: wsdl_reduce_workspace() bytes (double partials per workgroup, added by a
 *   finalize launch in fixed order; no atomics).  Two launches.
 * wsdl_surface_map: no counterpart in the reference.  surf_x[p] = (d2_out_x[p] == 1), int64, for two maps of n pixels: with
 *   d2_out from wsdl_edt (metric 0, border 1) these are the surface pixels of a mask, mask ^ binary_erosion(mask) with the
 *   4-neighbour footprint and a background border (medpy's surface), as a label map wsdl_edt takes.
 * wsdl_surface_stats: no counterpart in the reference; the sets behind the Hausdorff distance, its percentile and the
 *   average symmetric surface distance.  d2_out_a / d2_out_b: the planes above of masks A (prediction) and B (ground truth);
 *   to_a / to_b: d2_in of wsdl_edt (metric 0, border 0) of the two surface maps - the squared distance to the nearest surface
 *   pixel of A resp. B, WSDL_EDT_FAR where that surface is empty.  Direction 0 is A -> B: { to_b[p] : p on the surface of A },
 *   direction 1 is B -> A.  Per image b and direction d: n[b*2+d] = #surface pixels (int64), max_d2[b*2+d] = the largest
 *   squared distance (int32, 0 for an empty set), sum_d[b*2+d] = sum of sqrt((double)d2) (double; per-workgroup partials and
 *   a finalize launch in fixed order).  values (2,B,H,W) fp32 = (float)d2 on the surface, 0 elsewhere, and valid (2,B,H,W)
 *   uint8 = on the surface: what wsdl_kth_value ranks for a percentile.  H^2 + W^2 < 2^24, so (float)d2 is exact; 2 B H W <
 *   2^31.  ws: wsdl_surface_stats_workspace(B) bytes.  Two launches, no atomics. */
int wsdl_signed_distance(const int* d2_out, const int* d2_in, float* phi, int B, int HW, long long phi_batch_stride,
                         wsdl_stream_t stream);
int wsdl_boundary_loss_fwd_bwd(const float* logits, const float* phi, const int64_t* labels, const int* class_list, int K,
                               float* loss, float* dlogits, float* inv, const float* scale_dev, int B, int C, int H, int W,
                               long long ignore_index, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_surface_map(const int* d2_out_a, const int* d2_out_b, int64_t* surf_a, int64_t* surf_b, size_t n,
                     wsdl_stream_t stream);
size_t wsdl_surface_stats_workspace(int B);
int wsdl_surface_stats(const int* d2_out_a, const int* d2_out_b, const int* to_a, const int* to_b, int B, int H, int W,
                       long long* n_out, int* max_d2, double* sum_d, float* values, unsigned char* valid, void* ws,
                       size_t ws_bytes, wsdl_stream_t stream);

/* ---- overlap and focal losses (csrc/overlap_loss.hip) - no counterpart in the reference: its region losses are the two
 * Lovasz surrogates, and its pixel loss is the cross entropy.  Milletari et al., "V-Net", 3DV 2016 (soft Dice); Salehi et al.,
 * "Tversky loss function for image segmentation", MLMI 2017; Abraham & Khan, "A novel focal Tversky loss function", ISBI 2019;
 * Lin et al., "Focal loss for dense object detection", ICCV 2017.
 * Common: logits (B,C,H,W) fp32, labels (B,H,W) int64, s = softmax over C.  A pixel is valid when labels[p] != ignore_index.
 * Segments: the B images with per_image, else the whole batch is one segment (per_image: B <= 65535).  class_list: K distinct
 * ints in [0, C) on the HOST (copied into the launch by value; 1 <= K <= 32).  y_c(p) = 1 where p is valid and labels[p] == c;
 * a valid pixel whose label is not listed is background for every listed class.  The softmax and every product run in double
 * and each output is rounded once; per-workgroup double partials are added by a finalize launch in fixed order - no atomics,
 * bitwise reproducible.  With H W a multiple of 4 and 16-byte aligned pointers an item is four pixels, else one.
 * wsdl_overlap_workspace(segments, K): bytes of ws for the two calls below (0 for arguments out of range).
 * wsdl_overlap_sums: no counterpart in the reference.  sums[(segment * K + j) * 3 + {0, 1, 2}] (doubles) = for class
 *   c = class_list[j]:  I = sum_p s_c(p) y_c(p),  P = sum over valid p of s_c(p),  Y = sum_p y_c(p) (exact).  Two launches.
 * wsdl_tversky_fwd_bwd: no counterpart in the reference.  Per (segment, class), with N = I + smooth and
 *   D = I + alpha (P - I) + beta (Y - I) + smooth:  T = N / D, T = 1 where D == 0; the term is (1 - T)^gamma, exactly 0 with a
 *   zero gradient where 1 - T <= 0.  present_only drops the terms of classes with Y == 0 in their segment.
 *     loss = scale * mean over the kept (segment, class) terms, 0 when none is kept
 *     dlogits[b,j,p] = s_j (g_j - sum_c s_c g_c), g_c = a_c y_c(p) + b_c for a listed class, 0 for the others; exactly 0 at
 *       invalid pixels (may be null).  a, b per (segment, class) come from the finalize launch:
 *       d loss / d s_c(p) = -w [y D - N (alpha + y (1 - alpha - beta))] / D^2, w = scale gamma (1 - T)^(gamma - 1) / #terms;
 *       0 for dropped terms.  This is the COMPLETE gradient: the backward multiplies it by the upstream scalar only
 *       (wsdl_scale_by_device_scalar).
 *   scale = *scale_dev (a device float) or 1 when scale_dev is null.  alpha, beta, smooth >= 0, gamma > 0, all finite.
 *   alpha = beta = 1/2, gamma = 1 is the soft Dice loss 1 - (2 I + 2 smooth) / (P + Y + 2 smooth); gamma = 1 / (the paper's
 *   gamma) is the focal Tversky loss.  sums (optional, S K 3 doubles) receives the sums above.  No valid pixel: loss 0,
 *   gradient 0.  Three launches (two without dlogits), no host read.
 * wsdl_focal_fwd_bwd: no counterpart in the reference.  The contract of wsdl_softmax_ce_ex_fwd_bwd without smoothing: for pixel
 *   i with label y, class weights w (or null: 1), pixel weight p (or null: 1; p == 0 is an ignored pixel), q = 1 - s_y:
 *     l_i = p_i w[y] q^gamma (-log s_y)                                              (0 where y == ignore_index)
 *   reduction 0 (mean): *loss = sum_i l_i / sum_i p_i w[y_i] (gamma == 0 is the weighted cross entropy; 0/0 = NaN),
 *   *inv_count = 1 / that denominator; 1 (sum): *loss = sum_i l_i, *inv_count = 1; 2 (none): loss points at B*H*W floats,
 *   inv_count is not written.  dlogits (optional) = d l_i / d logits, UN-normalised, as there.  q is formed as the sum of the
 *   other classes' exponentials over the denominator, and the gradient factor gamma s_y q^(gamma-1) log s_y - q^gamma as
 *   q^gamma (gamma s_y (log s_y / q) - 1) with log s_y / q = -1 at q == 0: finite for every finite logit.  A label outside [0,C)
 *   that is not ignore_index: NaN.  gamma >= 0, finite.  ws: wsdl_reduce_workspace() bytes.  Two launches (one for reduction 2). */
size_t wsdl_overlap_workspace(int segments, int K);
int wsdl_overlap_sums(const float* logits, const int64_t* labels, const int* class_list, int K, double* sums, int B, int C,
                      int H, int W, int per_image, long long ignore_index, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_tversky_fwd_bwd(const float* logits, const int64_t* labels, const int* class_list, int K, float* loss, float* dlogits,
                         double* sums, const float* scale_dev, double alpha, double beta, double gamma, double smooth,
                         int per_image, int present_only, int B, int C, int H, int W, long long ignore_index, void* ws,
                         size_t ws_bytes, wsdl_stream_t stream);
int wsdl_focal_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, float* inv_count, int B, int C,
                       int H, int W, double gamma, long long ignore_index, const float* class_weight,
                       const float* pixel_weight, int reduction, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* ---- connected components of label maps, seeded region growing (csrc/components_grid.hip) - the reference has no such step -
 * wsdl_label_components: no counterpart in the reference (its only labelling is keep_largest's, one binary mask at a time).
 *   labels (B,H,W) int64, never written; comp (B,H,W) int32.  Two pixels of one image belong together if they are connected
 *   through pixels of the SAME label value, connectivity 8 or 4.  comp[p] = the raster index y W + x, within the image, of the
 *   first pixel of p's component in raster order (scipy.ndimage.label's order made position-independent); -1 where
 *   has_background is 1 and labels[p] == background (has_background 0: every value forms components).  area (optional,
 *   (B,H,W) int32, not comp): the pixel count of p's component at every pixel, 0 on background.
 *   Tiles of 64 x 32 pixels are labelled in LDS by one workgroup each, a second launch unites across the tile seams with a
 *   lock-free union (integer compare-and-swap: the larger root under the smaller, so parents only decrease and a component's
 *   root is its smallest raster index whatever the interleaving), a third replaces every parent by its root and a fourth
 *   spreads the areas.  No workgroup waits for another one, no host read, every parameter by value (a launch plan may hold
 *   the call), integer atomics only: bitwise reproducible.  ws: wsdl_label_components_workspace bytes, 4-byte aligned; its first
 *   int32 is the ERROR WORD: 0 after a complete run, 1 if a union gave up after 2^20 lost races (comp is then not valid) - the
 *   union loop is bounded instead of trusted.  Refused before any launch, without touching a device: non-positive sizes,
 *   B H W > 2^31 - 1 (the workspace query returns 0 for them), a connectivity other than 4 or 8.
 * wsdl_seeded_region_growing: no counterpart in the reference.  Deep seeded region growing (Huang et al., CVPR 2018) with a
 *   single-label seed map.  scores (B,C,H,W) fp32 (only compared), seeds (B,H,W) int64 (a value in [0,C) is a seed of that
 *   class, anything else is unseeded), thresh (C) fp32 either on the host (thresh_host: copied into the launch by value,
 *   C <= WSDL_SRG_THRESH_BY_VALUE) or in a device buffer (thresh_dev) - exactly one of the two; present (optional, (B,C) uint8):
 *   0 = a class the image cannot contain (null: all present).
 *     a(p)  = the first index of the largest score over the present classes
 *     p is a CANDIDATE of class a(p) iff scores[a(p)] > thresh[a(p)] (float32, strict); a NaN among the present scores of p, or
 *             no present class: a candidate of nothing
 *     the candidate map is labelled as above (8-connected, same class, non-candidates as background); a component GROWS iff
 *     one of its pixels carries a seed of the component's own class (candidates conduct also under a foreign seed)
 *     grown[p] (int64) = the seed where there is one (never overwritten), else the class of a grown component, else ignore_index
 *     counts[b,c] (int64 (B,C), on the device) = the pixels of image b with grown == c
 *   The seed flag per root is a plain byte store of 1 by every writer; counts are integer atomics: bitwise reproducible.  Six
 *   launches and a memset (one launch fewer for an image of one tile), no host read.  ws: wsdl_seeded_region_growing_workspace
 *   bytes, 16-byte aligned; its first int32 is the error word of the labelling.  Inputs are never written.
 * wsdl_balanced_seed_weights: no counterpart in the reference.  weights (B,H,W) fp32 from grown and counts: a pixel with a
 *   label l in [0,C) gets float(1.0 / double(B n)) - the division in double, rounded once - with n = counts[b,g] summed over
 *   the pixel's group g: balance 0 (fg_bg) the groups are {0} and {1..C-1}, 1 (class) every class by itself; 2 (none) the
 *   weight is 1.  Any other label: 0; a group without a pixel: 0 (the paper divides by zero there).  One launch. */
#define WSDL_SRG_THRESH_BY_VALUE 32
size_t wsdl_label_components_workspace(int B, int H, int W);
int wsdl_label_components(const int64_t* labels, int B, int H, int W, int connectivity, int has_background, long long background,
                          int* comp, int* area, void* ws, size_t ws_bytes, wsdl_stream_t stream);
size_t wsdl_seeded_region_growing_workspace(int B, int C, int H, int W);
int wsdl_seeded_region_growing(const float* scores, const int64_t* seeds, const float* thresh_host, const float* thresh_dev,
                               const uint8_t* present, int B, int C, int H, int W, long long ignore_index, int64_t* grown,
                               long long* counts, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_balanced_seed_weights(const int64_t* grown, const long long* counts, int B, int C, int H, int W, int balance, float* weights,
                               wsdl_stream_t stream);

/* ---- SLIC superpixels, superpixel pooling (csrc/slic.hip) - the reference has no such step --------------------------------
 * wsdl_slic: no counterpart in the reference.  SLIC (Achanta et al., TPAMI 2012; pixel-centric as in gSLIC) in fixed point on
 *   8-bit images (B,3,H,W) uint8, never written; the three channels are used as given.  All arithmetic is integer, `/` floors.
 *     grid        GH = max(1, (H + S/2) / S), GW likewise, K = GH GW; centre k = gy GW + gx starts at the pixel
 *                 cy = ((2 gy + 1) H) / (2 GH), cx = ((2 gx + 1) W) / (2 GW) with that pixel's colour.  A centre is five ints
 *                 (y, x, c0, c1, c2) in units of 1/16.  The home cell of pixel (y, x) is (min(GH-1, y GH / H), min(GW-1, x GW / W)).
 *     assignment  over the centres of the existing cells (hy + dy, hx + dx), dy, dx in {-1, 0, 1}:
 *                 D = S S sum_j (16 I_j - c_j)^2 + m m ((16 y - cy)^2 + (16 x - cx)^2) in 64 bits; smallest D, ties to the smallest k
 *     update      per k: n and the plain integer sums of y, x, I_0, I_1, I_2 (64-bit); each component (16 sum + n/2) / n; n = 0 keeps it
 *     loop        num_iter times assign, update; num_iter = 0 is one assignment against the initial centres.  raw (B,H,W) int32 is
 *                 the label map of the last assignment, centres (B,K,5) int32 the values after the last update.
 *     connectivity  raw is labelled 4-connected, every value, with areas (the kernels of wsdl_label_components).  The main component
 *                 of a label is its largest, the smallest first pixel on ties.  A component is an ORPHAN iff it is not its label's
 *                 main one, its area is < min_size and its first pixel is not pixel 0; an orphan with first pixel (y, x) is merged
 *                 into the component of (y, x-1), of (y-1, x) when x = 0 - a different component with a smaller first pixel, so a
 *                 chain of orphans ends at a kept component (more unions in the labelling's forest, then its flatten pass again;
 *                 chains of any length).  segments (B,H,W) int32: the rank, in raster order of first pixels, of the kept
 *                 component a pixel ends in; n_segments (B) int32, on the device, <= K + (H W) / min_size + 1.
 *   8 + L + max(1, 2 num_iter) launches, L = 4 labelling launches (3 when H <= 32 and W <= 64), no host read, every parameter by
 *   value, integer atomics only: bitwise reproducible.  ws: wsdl_slic_workspace bytes, 16-byte aligned; its first int32 is the
 *   labelling's error word (see wsdl_label_components).  Refused without touching a device: non-positive sizes, a side > 8192,
 *   B H W > 2^31 - 1, step outside [1, 128] (the workspace query returns 0 for these), compactness outside [1, 255],
 *   num_iter < 0, min_size < 1.
 * wsdl_superpixel_mean: no counterpart in the reference.  values (B,C,H,W) fp32, C <= 32; segments (B,H,W) int32 (a pixel whose id
 *   is outside [0, n_max) is not pooled).  count (B,n_max) int32 = the pixels of every segment; every value is quantised to
 *   q = llrint(double(clamp(v, -2^15, 2^15)) 2^24), the q are summed in 64-bit integers (on chip per tile first: one global atomic
 *   per tile, channel and touched segment) and mean (B,C,n_max) = float(double(sum) / (double(n) 2^24)); 0 where n = 0; NaN for an
 *   (image, channel, segment) that saw a NaN.  No float atomics: order-independent.  snapped (optional, (B,C,H,W)): every pixel's
 *   segment mean (0 at an id outside [0, n_max)).  Two launches and two memsets, three launches with snapped.
 *   ws: wsdl_superpixel_workspace(B, C, n_max) bytes, 8-byte aligned.
 * wsdl_superpixel_vote: no counterpart in the reference.  labels (B,H,W) int64; out (B,H,W) int64 = at every pixel the label in
 *   [0, num_classes) that most pixels of its segment carry, the smallest on ties; ignore_index for a segment without such a
 *   pixel.  num_classes <= 64; integer counts.  Three launches and a memset.  ws: 4 B n_max num_classes bytes
 *   (= wsdl_superpixel_workspace(B, num_classes, n_max) suffices). */
size_t wsdl_slic_workspace(int B, int H, int W, int step);
int wsdl_slic(const uint8_t* images, int B, int H, int W, int step, int compactness, int num_iter, int min_size, int* raw,
              int* centres, int* segments, int* n_segments, void* ws, size_t ws_bytes, wsdl_stream_t stream);
size_t wsdl_superpixel_workspace(int B, int C, int n_max);
int wsdl_superpixel_mean(const float* values, const int* segments, int B, int C, int H, int W, int n_max, float* mean, int* count,
                         float* snapped, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_superpixel_vote(const int64_t* labels, const int* segments, int B, int H, int W, int n_max, int num_classes,
                         long long ignore_index, int64_t* out, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* ---- AffinityNet: learned pairwise affinities, their loss and the CAM random walk (Ahn & Kwak, CVPR 2018; csrc/affinity.hip)
 * - the reference has no such step -
 * Features f (B,D,H,W) fp32, dense NCHW; labels (B,H,W) int64 on the same H x W.
 * Pair set: PSA's half disc of radius r, 2 <= r <= 8, in this order: first (0,x) for x = 1..r-1; then, for y = 1..r-1, every
 *   (y,x) with x = -(r-1)..r-1 and x^2 + y^2 < r^2.  P = 4 at r = 2 - (0,1),(1,-1),(1,0),(1,1) -, 34 at r = 5, 96 at r = 8
 *   (wsdl_affinity_num_pairs; 0 for a radius outside the range).
 *   A pair (p, q = p + o_j) is VALID iff q lies inside the image.  This is NOT PSA's crop of the "from" region (PSA takes its
 *   "from" pixels from the image shrunk by r - 1 on the left, right and bottom, so every pair it forms is complete): here every
 *   pixel is a "from" pixel and the pairs that leave the image do not exist.
 * Affinity: a(p,j) = exp(-(1/D) sum_d |f_d(p) - f_d(q)|) for a valid pair, exactly 0 for an invalid one; (B,P,H,W) fp32, plane j =
 *   offset j.  The channels are summed 8 at a time in float (in a fixed order), those partial sums in double; exp in double,
 *   one rounding of the result.
 * Loss (PSA's train_aff).  Kinds from the labels: both ends != ignore_index, equal and 0: bg-positive; equal and > 0: fg-positive;
 *   both != ignore_index and different: negative; anything else, or an invalid pair: not counted.  With the exact int64 counts
 *   n_bg, n_fg, n_neg over the whole batch and s_k = w_k / (n_k + eps):
 *     L = s_bg sum_bg -log(a + eps) + s_fg sum_fg -log(a + eps) + s_neg sum_neg -log(1 + eps - a)
 *   An empty kind contributes 0; no counted pair at all gives L = 0 and a zero gradient.  The sums run in double: one partial per
 *   workgroup, added in a fixed order by one workgroup; counts are integers; no float atomics - two calls give identical bits.
 * Gradient, closed form, gather form (no atomics): dL/df_d(p) = (1/D) sum over the up to 2 P full-disc neighbours q of
 *   c(p,q) sign(f_d(p) - f_d(q)) with the symmetric pair coefficient c = s_k a / (a + eps) for positives, c = -s_neg a / (1 + eps - a)
 *   for negatives; sign(0) = 0.  c is a float; the terms are summed 4 at a time in float (2 pairs, both orientations), those
 *   partial sums in double.
 * Transitions and walk: the neighbourhood of a pixel is itself (affinity 1) plus both orientations of every valid pair, at most
 *   2 P + 1 entries; w(p,q) = a(p,q)^beta / sum_q' a(p,q')^beta (beta > 0; the self term keeps the denominator >= 1); trans is
 *   (B,2P+1,H,W) fp32: plane 0 self, plane 1 + 2j offset j (q = p + o_j), plane 2 + 2j its reverse (q = p - o_j, weight
 *   a(q,j)^beta); 0 where q is outside.  One step is m'_c(p) = sum_q w(p,q) m_c(q), at most 2 P + 1 terms by fma in double in plane
 *   order, rounded once; num_iter steps equal PSA's cam @ T^t with T the column-normalised dense (A + I)^beta (elementwise
 *   power) and t = num_iter (PSA's defaults: beta 8, 256 steps).  No replicate padding: neighbours outside the image do not
 *   exist - neither their weight nor any score enters the sum, so an infinite score spreads as inf, not NaN.  A constant map is a
 *   fixed point.  Scores (B,C,H,W) fp32, 1 <= C <= 32.
 * Limits: 1 <= D <= 1024, H, W >= 1, H W <= 2^20.  Offsets and scalars reach the kernels by value: a launch plan may hold the calls.
 * wsdl_affinity_workspace: bytes of ws that suffice for every entry point below at this geometry (16-byte aligned); 0 outside
 *   the limits (host-side, no device touched).
 * wsdl_affinity_pair_affinity: aff (B,P,H,W).  One launch.
 * wsdl_affinity_pair_affinity_backward: dfeat (B,D,H,W) = dL/df from daff = dL/da (B,P,H,W) and aff.  One launch.
 * wsdl_affinity_pair_counts: counts_out[3] int64 = n_bg, n_fg, n_neg.  Two launches.
 * wsdl_affinity_loss: counts, forward with the per-kind partial sums and the pair coefficients, the finalize (loss: one float) and,
 *   if dfeat is not null, the gradient (B,D,H,W): five launches.  counts_out (optional): int64[3].
 * wsdl_affinity_transitions: trans (B,2P+1,H,W) from aff.  One launch.
 * wsdl_affinity_random_walk: num_iter steps from scores to out, one launch per step over the whole batch, ping-pong between two
 *   buffers carved from ws (not needed for num_iter < 2); the result lands in out for every num_iter; num_iter = 0 copies;
 *   scores is never written; out must not overlap scores or trans.  (A second path - one launch for all steps, one workgroup
 *   per (image, channel) with its plane in LDS, identical bits - was built and measured: 2009 against 1915 us at scores
 *   (16,2,32,32) and 7859 against 1938 us at (8,2,64,64), 256 steps; not faster at either, so it is not shipped.) */
size_t wsdl_affinity_workspace(int B, int D, int C, int H, int W, int radius);
int wsdl_affinity_num_pairs(int radius);
int wsdl_affinity_pair_affinity(const float* feat, int B, int D, int H, int W, int radius, float* aff, wsdl_stream_t stream);
int wsdl_affinity_pair_affinity_backward(const float* feat, const float* aff, const float* daff, float* dfeat, int B, int D, int H,
                                         int W, int radius, wsdl_stream_t stream);
int wsdl_affinity_pair_counts(const long long* labels, int B, int H, int W, int radius, long long ignore_index,
                              long long* counts_out, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_affinity_loss(const float* feat, const long long* labels, float* loss, float* dfeat, long long* counts_out, int B, int D,
                       int H, int W, int radius, long long ignore_index, double w_bg, double w_fg, double w_neg, double eps, void* ws,
                       size_t ws_bytes, wsdl_stream_t stream);
int wsdl_affinity_transitions(const float* aff, float* trans, int B, int H, int W, int radius, double beta, wsdl_stream_t stream);
int wsdl_affinity_random_walk(const float* trans, const float* scores, float* out, int B, int C, int H, int W, int radius,
                              int num_iter, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* ---- IRN boundary paths: affinities along the line between two pixels, their loss and the seed of the boundary CAM walk
 * (Ahn, Cho & Kwak, CVPR 2019; csrc/boundary_affinity.hip) - the reference has no such step; this is the project's definition -
 * One class-boundary map e (B,H,W) fp32 in [0,1], or its logits z; labels (B,H,W) int64 on the same H x W.
 * Pairs: the half disc, the plane order and the validity rule of the AffinityNet block, 2 <= r <= 8.
 * Paths: for the offset o_j = (dy,dx), dy >= 0, S_j is every integer point (y,x) with 0 <= y <= dy, min(0,dx) <= x <= max(0,dx) and
 *   (dy x - dx y)^2 < dy^2 + dx^2 (integers: the distance to the line is below 1, IRN's "thick" line), in raster order of (y,x).
 *   Both ends are members.  r = 2: 12 points over the 4 offsets, longest path 4; r = 5: 242, 11; r = 8: 1078, 16; the shortest
 *   path has 2 points.  S_(1,-1) = (0,-1),(0,0),(1,-1),(1,0).  A path never leaves the rectangle between its ends, so every
 *   point of a valid pair lies inside the image.
 * Affinity: for a valid pair m = max over s in S_j of e(p + s) and a(p,j) = 1.0f - m, one float subtraction; exactly 0 for an
 *   invalid pair (IRN pads the boundary map with 1).  arg(p,j), uint8: the FIRST point in path order that attains the maximum; a NaN
 *   on the path gives NaN and arg is the first NaN (torch.max(dim)); 0 for an invalid pair.  A valid pair may have affinity 0 or 1.
 *   The result equals a float32 evaluation bit for bit.  aff (B,P,H,W) fp32, arg (B,P,H,W) uint8.
 * Backward: dedge(r) = - sum of daff(p,j) over every (j,t) with p = r - S_j[t], the pair (p,j) valid and arg(p,j) = t: gather
 *   form, no atomics; the terms are added in (j,t) order in double and rounded once.
 * Loss (IRN's pos_aff_loss / neg_aff_loss on the logits z of the boundary head): kinds, exact int64 counts and s_k = w_k / (n_k +
 *   eps) as in the AffinityNet block.  zmax and its arg index over the path of the LOGITS (the sigmoid is monotone); a =
 *   sigmoid(-zmax) = 1 / (1 + exp(zmax)) and 1 - a = sigmoid(zmax) = 1 / (1 + exp(-zmax)), each formed directly in double, never by
 *   a subtraction:
 *     L = s_bg sum_bg -log(a + eps) + s_fg sum_fg -log(a + eps) + s_neg sum_neg -log(sigmoid(zmax) + eps)
 *   An empty kind contributes 0; no counted pair at all gives L = 0 and a zero gradient.  The pair coefficient dL/dzmax is c = s_k a (1 -
 *   a) / (a + eps) for positives and c = -s_neg a (1 - a) / ((1 - a) + eps) for negatives, a float; it goes to the arg pixel only:
 *   dL/dz(r) = sum of c(p,j) over the same (j,t) as above, in double, one rounding; (B,H,W) fp32.  The sums of the loss run in
 *   double: one partial per workgroup, added in a fixed order by one workgroup; no float atomics - two calls give identical bits.
 * Seed: out_c = scores_c * (1 - e), two float operations, for scores (B,C,H,W), 1 <= C <= 32: IRN's propagate_to_edge damps the seed
 *   on predicted boundaries; the walk itself is wsdl_affinity_transitions / wsdl_affinity_random_walk on aff, unchanged.
 * Limits: H, W >= 1, H W <= 2^20.  The path table is part of the code; every other value reaches the kernels by value or
 *   through ws: a launch plan may hold the calls.
 * wsdl_path_affinity_workspace: bytes of ws that suffice for wsdl_path_affinity_loss (16-byte aligned); 0 outside the limits
 *   (host-side, no device touched).
 * wsdl_path_affinity_paths: host-side, no device touched: the total number of path points at this radius, 0 for a radius outside
 *   the range; lengths[P] (optional) receives the path lengths in plane order, points_yx[2 total] (optional) the points as y, x.
 * wsdl_path_affinity: aff and, if arg is not null, arg.  One launch.
 * wsdl_path_affinity_backward: dedge (B,H,W) from daff and arg.  One launch.
 * wsdl_path_affinity_loss: counts (two launches), forward with the per-kind partial sums, the pair coefficients and the arg indices
 *   in ws, the finalize (loss: one float) and, if dlogits is not null, the gather (B,H,W): five launches.  counts_out (optional):
 *   int64[3].
 * wsdl_path_affinity_seed: one launch; out may be scores. */
size_t wsdl_path_affinity_workspace(int B, int H, int W, int radius);
int wsdl_path_affinity_paths(int radius, int* lengths, int* points_yx);
int wsdl_path_affinity(const float* edge, int B, int H, int W, int radius, float* aff, uint8_t* arg, wsdl_stream_t stream);
int wsdl_path_affinity_backward(const float* daff, const uint8_t* arg, float* dedge, int B, int H, int W, int radius,
                                wsdl_stream_t stream);
int wsdl_path_affinity_loss(const float* logits, const long long* labels, float* loss, float* dlogits, long long* counts_out, int B,
                            int H, int W, int radius, long long ignore_index, double w_bg, double w_fg, double w_neg, double eps,
                            void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_path_affinity_seed(const float* edge, const float* scores, float* out, int B, int C, int H, int W, wsdl_stream_t stream);

/* ---- GroupNorm (Wu & He, ECCV 2018; torch.nn.functional.group_norm) with an optional fused ReLU, and its complete backward
 * (csrc/group_norm.hip) - the reference has no such layer; IRN's boundary head puts GroupNorm(4, 32) behind its reductions -
 * x, y, dy, dx (B,C,HW) fp32 dense; G groups of C / G consecutive channels; gamma, beta (C) fp32, each may be null (1 and 0).
 * With n = (C / G) HW, over group (b,g): mean = sum x / n, var = sum (x - mean)^2 / n (biased), rstd = 1 / sqrt(var + eps);
 *   y = (x - mean) rstd gamma[c] + beta[c], then max(., 0) if relu (+0 for -0 and for a NaN, as wsdl_affine_act_fwd).
 * Train and eval are the same function; there are no running statistics.  A group of one element is accepted (torch refuses it):
 * y = beta and dx = 0 exactly.  A constant group has var = 0 and stays finite for eps > 0.  A NaN poisons its own group only.
 * Backward, with m the ReLU mask (y > 0: 0 at exactly 0, as ATen; 1 without relu), g = dy m gamma[c], xhat = (x - mean) rstd:
 *   dx = rstd (g - mean_grp(g) - xhat mean_grp(g xhat)),  dgamma[c] = sum_{b,hw} dy m xhat,  dbeta[c] = sum_{b,hw} dy m.
 *   dx, dgamma and dbeta may each be null: only what is asked for is computed.  accumulate_param_grads: dgamma / dbeta receive
 *   old + (float)sum, one float addition, instead of (float)sum.
 * Arithmetic: the group statistics and every backward sum are accumulated in double.  The second moment is taken about a sample
 *   of the data (per chunk: sum (x - K)^2 with K the chunk's first element) and the chunks' (n, mean, M2) are combined; nothing
 *   is formed as E[x^2] - E[x]^2.  save_mean / save_rstd (B,G) are DOUBLE: rounding the mean of data at offset 1000 to a float
 *   moves xhat by up to 6e-5 at sigma = 0.5, the size of the whole float32 error there.  Every element of y and dx is computed in
 *   double and rounded once.  All partials are combined in a fixed order, no atomics: two calls give identical bits, and so
 *   does a replayed plan.
 * Parallelism: a plane (b,c) is cut into P chunks of L floats (L a multiple of 1024, >= 2048, chosen so that B C P is about 1024
 *   where the tensor allows it); one 256-thread workgroup per chunk in every pass; per-chunk partials in ws; one wave per group /
 *   per channel combines them.  float4 accesses where HW % 4 == 0 and the pointers are 16-byte aligned, one float per lane
 *   otherwise.
 * Limits, each refused with an error: B, C, HW >= 1; G >= 1 and C % G == 0; B C HW <= 2^31 - 1; ws_bytes >= the workspace
 *   query, ws 8-byte aligned; eps finite and >= 0; relu in the backward needs y.
 * wsdl_group_norm_workspace: bytes of ws that suffice for either direction; 0 for a bad geometry (host-side, no device touched).
 * wsdl_group_norm_fwd: three launches (chunk statistics, one wave per group, apply).  y may be x.
 * wsdl_group_norm_bwd: y is read only if relu.  Three launches (chunk sums, one wave per group and per channel, dx), two without
 *   dx.  No host read and no allocation in either: a launch plan may hold both. */
size_t wsdl_group_norm_workspace(int B, int C, int HW, int G);
int wsdl_group_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, double* save_mean, double* save_rstd, int B,
                        int C, int HW, int G, double eps, int relu, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_group_norm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const double* save_mean,
                        const double* save_rstd, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int G, int relu,
                        int accumulate_param_grads, void* ws, size_t ws_bytes, wsdl_stream_t stream);

/* ---- multi-scale fusion: scaled + mirrored batches and the fusion of their maps (csrc/multiscale.hip) - the reference has no
 * such step.  PSA / IRN build a CAM as the sum over scales and a horizontal flip, DeepLab-family results are reported with
 * multi-scale + flip inference; these are the launches AROUND the network.  fp32 planes, dense NCHW, all bilinear arithmetic
 * is wsdl_bilinear_fwd's (align_corners = false), bit for bit.
 * wsdl_scale_flip: x (B,C,H,W) -> y ((1 + flip) B, C, h, w), one launch.  Images [0, B) are wsdl_bilinear_fwd's result
 *   (h == H and w == W: a copy), images [B, 2B) the same planes mirrored left-right - resize THEN mirror.
 * wsdl_multiscale_fuse: up to WSDL_MS_MAX_SOURCES sources -> one (B,C,H,W) map, one launch.  Source s is (B,C,h_s,w_s), or
 *   (2B,C,h_s,w_s) with `mirrored`: images [B, 2B) then belong to mirrored inputs.  A MEMBER is a source's plain half or its
 *   mirrored half, in source order, plain before mirrored.  Member value at output pixel (b,c,oh,ow):
 *   act(bilinear_{(h_s,w_s)->(H,W)}(plane)[oh, x]) with x = ow for a plain half and W - 1 - ow for a mirrored one (it is
 *   un-mirrored AFTER the resize); h_s == H and w_s == W reads plane[oh, x] itself.  act: 0 none; 1 softmax over the C values
 *   of the member AT that output pixel (float maximum m, e_c = expf(v_c - m), double sum over c in order, e_c * (1 / sum));
 *   2 sigmoid (e = expf(-|v|), 1 / (1 + e) or e / (1 + e), in double).  reduce: 0 weighted mean - sum over the members of
 *   (weight_s / sum of all members' weights) * value, in double, a source of weight 0 takes no part; 1 maximum (weights are
 *   not read; a NaN member makes the result NaN).  The double is rounded once.  Outputs, each may be null but not all:
 *   scores (B,C,H,W); labels (B,H,W) int64 and conf (B,H,W) - wsdl_pamr_labels' rule on the ROUNDED scores: C >= 2 the index
 *   of the first maximum, ignore_index where it is < min_conf, conf = that maximum; C == 1: score >= thresh, conf = the score.
 *   Labels need no score planes.  1 <= C <= WSDL_MS_MAX_CHANNELS (C <= 24: a pixel's channels stay in registers; beyond, the
 *   softmax statistics take a first pass over the taps).  No atomics: bitwise reproducible.  The sources are copied into the
 *   launch BY VALUE: a launch plan may hold the call.  No output may overlap a source.
 * wsdl_plane_max_normalize: out[b] = x[b] / max(x[b]) over the per_image values of image b, v / max in double rounded once;
 *   an image whose maximum is <= 0, infinite or NaN (any NaN in it) is copied unchanged.  mask (optional, uint8, the shape of
 *   x): out >= thresh && out > 0 (the rule of wsdl_layercam_epilogue's mask).  out may be x.  A memset and two launches; the
 *   maximum goes through an integer atomic max on float bits: bitwise reproducible.  ws: wsdl_plane_max_workspace(B) bytes
 *   (0 for B outside [1, 65535]). */
#define WSDL_MS_MAX_SOURCES 8
#define WSDL_MS_MAX_CHANNELS 64
typedef struct wsdl_ms_source {
    const float* data;
    int h, w;
    float weight;   /* >= 0, finite */
    int mirrored;   /* != 0: the leading dimension is 2B */
} wsdl_ms_source;
int wsdl_scale_flip(const float* x, float* y, int B, int C, int H, int W, int h, int w, int flip, wsdl_stream_t stream);
int wsdl_multiscale_fuse(const wsdl_ms_source* sources, int n_sources, int B, int C, int H, int W, int activation, int reduce,
                         float* scores, long long* labels, float* conf, float thresh, float min_conf, long long ignore_index,
                         wsdl_stream_t stream);
size_t wsdl_plane_max_workspace(int B);
int wsdl_plane_max_normalize(const float* x, float* out, unsigned char* mask, int B, long long per_image, float thresh, void* ws,
                             size_t ws_bytes, wsdl_stream_t stream);

/* ---- refine_pseudo_mask inner step (TraditionalModel/AlternatingDirectionCutLoss.py:736-757) -
 * KL(softmax(X) || S) with log(X+1e-8), reduction 'batchmean', and its gradient wrt softmax(X). */
int wsdl_kl_div_fwd_bwd(const float* xn, const float* s, float* loss, float* dxn, size_t n, int batch,
                        void* ws, size_t ws_bytes, wsdl_stream_t stream);
/* Batched refinement: the same step for N images at once, every per-image scalar kept on the
 * device.  kl_div_per_image: loss[i] = sum_i target*(log target - log(xn+1e-8)) over image i (reduction
 * 'batchmean' of the reference's (1,C,H,W) call), dxn = -target/(xn+1e-8).  refine_combine:
 * out = dkl + lambda*kl_i/(nc_scale*nc_i + 1e-6) * nc_scale * dnc  - the reference's dynamic weight
 * (AlternatingDirectionCutLoss.py:748) without its two host synchronisations per step. */
int wsdl_kl_div_per_image_fwd_bwd(const float* xn, const float* s, float* loss, float* dxn, int N,
                                  size_t per_image, void* ws, size_t ws_bytes, wsdl_stream_t stream);
int wsdl_refine_combine(const float* dkl, const float* dnc, const float* kl, const float* nc, float lambda,
                        float nc_scale, float* out, int N, size_t per_image, wsdl_stream_t stream);
/* softmax over C of (B,C,HW) and its backward */
int wsdl_softmax_fwd(const float* x, float* y, int B, int C, int HW, wsdl_stream_t stream);
int wsdl_softmax_bwd(const float* y, const float* dy, float* dx, int B, int C, int HW, wsdl_stream_t stream);

/* ---- Class prototypes: masked feature pooling, prototype similarity maps and the pixel-to-prototype contrast loss
 * (SIPE: Chen et al., CVPR 2022; Du et al., CVPR 2022; Wang et al., ICCV 2021; csrc/prototype.hip) - the reference has no such
 * step; this is the project's definition.  feat is float (B,D,H,W), dense, D <= 2048, H W <= 2^20, K <= 32 classes.
 * Norms: n(x) = max(sqrt(sum_d x_d^2), eps) and u_p = f_p / n(f_p) (F.normalize).  A segment s is one image (S = B) or the whole
 * batch (S = 1).
 *   Prototypes: mass[s,k] = sum of w_p (pixel_weight, or 1 when it is null) over the pixels of s with labels_p == k; labels equal to
 *   ignore_index or outside [0,K) are not pooled; proto[s,k,:] = sum w_p x_p / mass[s,k] with x_p = u_p (normalize) or f_p, exactly 0
 *   where the mass is not > 0.  Sums in double, every (s,k,d) sum owned by one wave per image, the images added in order: no
 *   atomics, the same bits on every call.  mass is float: exact up to 2^24 for unit weights.
 *   Similarity: sim[b,k,p] = <u_p, q_k>, q_k = proto[s(b),k,:] / n(proto[s(b),k,:]) (a zero prototype gives 0); activation 0: as it
 *   is, 1: max(sim, 0), 2: the softmax over the classes marked in present (S,K) uint8 (null: all) of sim / temperature, exactly 0
 *   for an absent class.
 *   Contrast: z_{p,k} = sim[b,k,p] / temperature over the present classes, l_p = -log softmax(z_p)[y_p]; a pixel counts iff its
 *   label is not ignore_index and its class is present; a label outside [0,K) other than ignore_index gives NaN.  reduction 0:
 *   loss = sum w_p l_p / sum w_p over the counted pixels (0 without one), 1: the sum, 2: loss is (B,H,W), w_p l_p per pixel (0
 *   where not counted).  dfeat (null: forward only, the same loss bits) receives, with g_k = w_p (softmax_k - [k == y_p]),
 *   v = sum_k g_k q_k / temperature and c = sum_k g_k sim_k / temperature: (v - c u_p) / n(f_p), or v / eps where the norm is
 *   below eps; exact zeros at a pixel that does not count.  The prototypes are constants.  inv (one float, may be null)
 *   receives the factor the mean's gradient still needs, 1 / sum w_p (0 without a counted pixel; 1 for the sum).
 *   Bank: bank[k,:] = m bank[k,:] + (1 - m) proto[k,:] and count[k] += 1 for the classes with mass[k] > 0; a class whose count was
 *   0 takes proto[k,:] as it is; the others are untouched.
 * wsdl_proto_workspace: bytes of ws that suffice for every entry point below at this geometry (16-byte aligned); 0 outside the
 * limits.  wsdl_proto_pool: three launches; wsdl_proto_similarity: two; wsdl_proto_contrast: two and the one-workgroup finalize
 * (none for reduction 2); wsdl_proto_ema: one.  No host read, every parameter by value: a launch plan can hold them. */
size_t wsdl_proto_workspace(int B, int D, int K, int H, int W);
int wsdl_proto_pool(const float* feat, const long long* labels, const float* pixel_weight, float* proto, float* mass, int B, int D,
                    int H, int W, int K, int per_image, int normalize, long long ignore_index, double eps, void* ws, size_t ws_bytes,
                    wsdl_stream_t stream);
int wsdl_proto_similarity(const float* feat, const float* proto, const unsigned char* present, float* out, int B, int D, int H, int W,
                          int K, int S, int activation, double temperature, double eps, void* ws, size_t ws_bytes,
                          wsdl_stream_t stream);
int wsdl_proto_contrast(const float* feat, const float* proto, const long long* labels, const unsigned char* present,
                        const float* pixel_weight, float* loss, float* dfeat, float* inv, int B, int D, int H, int W, int K, int S,
                        long long ignore_index, double temperature, double eps, int reduction, void* ws, size_t ws_bytes,
                        wsdl_stream_t stream);
int wsdl_proto_ema(float* bank, long long* count, const float* proto, const float* mass, int K, int D, double momentum,
                   wsdl_stream_t stream);

/* ---- launch plans: the reference's training / CAM loops as one host call per iteration ------------------------------
 * The reference runs its loops statement by statement from Python (one training iteration:
 * TraditionalModel/AlternatingDirectionCutLoss.py:693-703 = SegmentationModel.py:96-113; one CAM batch:
 * TraditionalModel/PsuedoMasks.py:47-62); on this path an iteration is ~520 kernel launches on three streams, 10-14 ms of
 * host time through Python + ctypes against 18.7 ms on the GPU.  A plan records the launches of ANY sequence of the calls of
 * this header once - function, grid, block, LDS bytes, stream and a private copy of every argument value, plus the
 * cross-stream dependencies made through the wsdl_event_* / wsdl_stream_wait_* calls below - while the sequence runs in the
 * ordinary way, and wsdl_plan_replay issues them again from one C loop (csrc/plan.hip).  Same kernels, same arguments,
 * same order per stream: the results are the recorded sequence's, bit for bit.
 *   - one recording at a time PER HOST THREAD (the recording state is thread-local): other threads may call into the
 *     library meanwhile - their launches run normally and are not part of this thread's plan - and may record plans of
 *     their own; wsdl_set_option is refused while any thread records;
 *   - the caller keeps every buffer the sequence touched alive and at its address for the plan's lifetime, and anything
 *     that varies from replay to replay on the device (wsdl_adam_step's step_dev, wsdl_dropout_fwd's counter);
 *   - wsdl_lovasz_softmax_fwd_bwd, wsdl_lovasz_hinge_fwd_bwd and wsdl_lovasz_softmax_classes_fwd_bwd (rocPRIM launches
 *     kernels of its own) poison a recording: wsdl_plan_end fails;
 *   - wsdl_plan_mark(tag) cuts the plan into segments: wsdl_plan_replay_segment(plan, k) replays segment k (0 .. marks),
 *     so the host can do its own work (a gradient collective) at the places it did while recording. */
int wsdl_plan_begin(void);
int wsdl_plan_recording(void);                       /* 1 between begin and end */
int wsdl_plan_end(void** plan_out);                  /* error (and no plan) if the sequence cannot be replayed */
int wsdl_plan_abort(void);                           /* drop the recording in progress */
int wsdl_plan_mark(long long tag);
int wsdl_plan_pause(void);                           /* host section: what the library is asked to do until wsdl_plan_resume is NOT */
int wsdl_plan_resume(void);                          /* recorded (the host repeats it itself between the segments of a replay)      */
int wsdl_plan_poison(const char* why);               /* the caller did something between begin and end that a replay would miss */
int wsdl_plan_replay(void* plan);
int wsdl_plan_replay_segment(void* plan, int segment);
/* diagnostic twin of wsdl_plan_replay: host microseconds inside the runtime and the count per kind of operation, six
 * entries each (0 kernel launch, 1 memset, 2 stream-waits-for-stream, 3 event record, 4 event wait, 5 mark) */
int wsdl_plan_replay_timed(void* plan, double* us_by_kind, long long* n_by_kind);
int wsdl_plan_stats(void* plan, long long* kernels, long long* memsets, long long* stream_waits, long long* events,
                    long long* marks);
long long wsdl_plan_mark_tag(void* plan, int i);
int wsdl_plan_destroy(void* plan);
/* Stream ordering through the library, so that a plan sees it: events (no timing), "stream waits for event", and
 * "waiter waits for everything enqueued on waited so far".  Outside a recording they are the plain runtime calls. */
int wsdl_event_create(void** ev);
int wsdl_event_destroy(void* ev);
int wsdl_event_record(void* ev, wsdl_stream_t stream);
int wsdl_stream_wait_event(wsdl_stream_t stream, void* ev);
int wsdl_stream_wait_stream(wsdl_stream_t waiter, wsdl_stream_t waited);
/* The few stream-ordered helpers a training step used the tensor library's own kernels for (a plan records launches of
 * THIS library only): memset, *p += delta for a device int32 / int64 (Adam's step number, the dropout call counters),
 * out[i] = a[i] * b[i] (the loss scale of the cross-entropy backward), y = min(x, hi) for int64 labels
 * (torch.clamp(masks, max=1), reference SegmentationModel.py:100). */
int wsdl_memset_async(void* dst, int value, size_t bytes, wsdl_stream_t stream);
int wsdl_add_int(void* p, int is64, long long delta, wsdl_stream_t stream);
int wsdl_mul(const float* a, const float* b, float* out, int n, wsdl_stream_t stream);
int wsdl_clamp_max_i64(const long long* x, long long* y, long long n, long long hi, wsdl_stream_t stream);
/* Weighted loss terms without the tensor library: out[0] = w * mean(x[0..n)) (the "0.1 * ncut" / "0.1 * boundary.mean()" of the
 * reference's combined losses, AlternatingDirectionBoundaryLoss.py:196-200; fixed summation order) and its gradient
 * out[i] = g[0] * c (c = w / n).  The sum of terms is wsdl_add. */
/* Range sentinel of the fp16x2 arithmetic.  wsdl_set_option("range_sentinel", 1) declares that every y_amax / dx_amax handed
 * to wsdl_bn_train_fwd / wsdl_bn_train_bwd points at TWO floats (8-byte aligned): [0] receives max|tensor| as before, [1] the smallest non-zero
 * maximum of any CHANNEL of the tensor (the channel-resident kernels run one workgroup per channel),
 * kept as the bitwise complement of its float bits (a zeroed pair = nothing published).  The convolutions scale a tensor by
 * ONE power of two, so a region 2^E below the tensor's maximum is computed to 2^-(38-E) of its own maximum - past the 1e-3
 * of the parity bar from E ~ 29.  wsdl_range_check reduces npairs such pairs: out[0] = the largest log2(max / min channel
 * maximum), out[1] = the number of pairs beyond limit_log2 (25: the safe range), out[2] = pairs looked at.  `out` may be
 * pinned host memory: the host reads it a step later, without a synchronisation, and selects conv_arith = 2 (the guard). */
int wsdl_range_check(const float* pairs, int npairs, int limit_log2, float* out, wsdl_stream_t stream);
int wsdl_scale_mean(const float* x, int n, float w, float* out, wsdl_stream_t stream);
int wsdl_scale_fill(const float* g, float c, float* out, int n, wsdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WSDL_HIP_H */
