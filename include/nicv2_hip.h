/*
 * nicv2_hip.h - C ABI of the MI355X (gfx950) implementation of the reference's per-sample hot path:
 *               feature-grid gather + positional encoding + tiny GELU MLP, forward and backward.
 *
 * The reference (21K1113/Neural_Image_Compression_V2) is pure Python and has no FFI of its own; the
 * boundary is the Python call surface of Projects/fp_def.py, Projects/utils.py, Projects/models.py and
 * the create_decoder_input / ColorDecoder / decode_image part of Projects/image_compression.py.
 * Every entry point below names the reference lines it replaces.  The host mirror of those Python
 * signatures lives in neural_image_compression_v2_amd/ and binds this library with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host; tensors are dense fp32.
 *  - a grid is [C, (Z,) Y, X] like the reference (fp_def.py:54,76); the FIRST sample axis ("x",
 *    coord[0]) walks the LAST grid axis (fp_def.py:81-112).  All per-axis arrays in this header are
 *    given in sample-axis order (x, y, z).
 *  - samples of a crop are numbered x-outer ... z-inner, crops back to back (fp_def.py:124-129,
 *    image_compression.py:97); N = num_crops * extent[0] * extent[1] * extent[2].
 *  - decoder weights are nn.Linear layout [out, in] row-major (image_compression.py:57-64).
 *  - all functions are asynchronous on `stream` (a hipStream_t passed as void*), allocate nothing and
 *    never synchronise, so a caller may capture them into a hipGraph.
 *  - return value: 0 on success, a positive hipError_t from the runtime, or a negative NIC_E_* code.
 */
#ifndef NICV2_HIP_H
#define NICV2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIC_ABI_VERSION 9

enum {
    NIC_OK = 0,
    NIC_E_NULL = -1,        /* required pointer is null */
    NIC_E_UNSUPPORTED = -2, /* dim / method / channels / hidden combination has no kernel */
    NIC_E_SHAPE = -3,       /* extents, node counts or origins inconsistent (index would leave the grid) */
    NIC_E_WORKSPACE = -4,   /* workspace smaller than nic_workspace_bytes() */
    NIC_E_ARG = -5          /* other invalid argument */
};

/* pe_mode */
enum { NIC_PE_TRIANGULAR = 0 /* utils.py:211-227 */, NIC_PE_SINUSOIDAL = 1 /* utils.py:198-208 */ };
/* g1_weight_mode */
enum {
    NIC_G1_REFERENCE = 0,  /* bilinear in 2D; the reference's permuted trilinear products in 3D (fp_def.py:176-183) */
    NIC_G1_TEXTBOOK = 1,   /* true trilinear */
    NIC_G1_UNWEIGHTED = 2  /* plain corner sum: what the reference does when step_number == 2 (fp_def.py:136) */
};
/* noise_mode */
enum {
    NIC_NOISE_NONE = 0,
    NIC_NOISE_TENSOR = 1,  /* caller supplies the [N, Cin] noise (parity with torch.rand_like, image_compression.py:250) */
    NIC_NOISE_KERNEL = 2   /* generated in-kernel: Threefry-4x32-12 keyed by (seed, offset, global sample id, channel block) */
};

/* Geometry of one launch: which grid pair, which samples.  Mirrors the arguments of
 * create_g0_g1 / create_g0_g1_3d / create_g0_g1_3d_v2 (fp_def.py:115,148,187) and of
 * create_decoder_input_2d/_3d/_3d_v2 (image_compression.py:71,103,137). */
struct nic_step_tail;
typedef struct nic_path_desc {
    int32_t dim;             /* 2 or 3 */
    int32_t method;          /* 1: 2D.  3: 3D, 8 raw G0 corners.  4: 3D, 4 tetrahedral G0 corners (fp_def.py:107-112) */
    int32_t channels;        /* FEATURE_PYRAMID_CHANNELS (var2.py:68) */
    int32_t pe_channels;     /* PE_CHANNELS (var2.py:69) */
    int32_t hidden;          /* HIDDEN_LAYER_CHANNELS (var2.py:72) */
    int32_t pe_mode;         /* NIC_PE_* */
    int32_t g1_weight_mode;  /* NIC_G1_* */
    int32_t log2_step;       /* step_number = 2^log2_step = 2^(mip - 2(fl+1))  (image_compression.py:79) */
    float lod_value;         /* value of the LOD channel = mip_level (image_compression.py:95) */
    int32_t num_crops;
    int32_t extent[3];       /* samples per axis of one crop (sample_number); extent[2] = 1 in 2D */
    int32_t g0_nodes[3];     /* nodes per axis of G0 = fp[2*fl]  (x, y, z order) */
    int32_t g1_nodes[3];     /* nodes per axis of G1 = fp[2*fl+1] */
    float pe_div[8];         /* sinusoidal div_term, fp32, pe_channels/2 entries (utils.py:202) */
    int32_t noise_mode;      /* NIC_NOISE_* */
    int32_t num_bits;        /* FP_BITS: noise amplitude 2^-num_bits (image_compression.py:250) */
    uint64_t noise_seed;
    uint64_t noise_offset;  /* e.g. the training step */
    int64_t sample_base;     /* global id of this launch's sample 0 (data-parallel shards: keeps the noise world-size invariant) */
    float loss_scale;        /* 1 / (3 * N_global): the MSELoss mean (image_compression.py:259) */
    int32_t flags;           /* NIC_FLAG_* (0 is always valid) */
    int32_t passes;          /* training entry points: every crop is sampled `passes` times in one launch (0 and 1 = once); pass k of
                              * crop c has the sample ids (c * passes + k) * n_per_crop + ..., i.e. its own noise and its own target /
                              * dy rows (N = num_crops * passes * n_per_crop) - the same result as listing the crop `passes` times, but
                              * a cell's gradients are summed over all passes before they go to memory (stripe-sharded multi-GPU steps).
                              * Every other entry point: 0 or 1. */
    int32_t dz_scale_log2;   /* NIC_FLAG_FP16 only: dZ is carried as 2^dz_scale_log2 x dZ.  0: nic_fused_forward_backward / _img / _img_dev choose it from
                              * loss_scale (2 loss_scale 2^k in [4, 8)); nic_fused_backward_dy takes 2^0 - pass the exponent that brings the incoming
                              * dY to O(1) (a mean-squared-error dY is 2 (y - t) / (3 N): k = round(log2(3 N)) + 1) */
    int32_t max_workgroups;  /* 0: the launch may fill the chip (one persistent workgroup per CU, two for inference).  n > 0: at most n
                              * workgroups (rounded down to a multiple of 8, at least 8): independent fits launched on separate
                              * streams (BASELINE config 5) then share the CUs side by side instead of queueing behind each other's
                              * persistent grids. */
    const struct nic_step_tail *tail; /* training entry points (nic_fused_forward_backward, _img, _img_dev, nic_fused_backward_dy,
                              * nic_fused_ml_forward_backward): null, or the optimiser step that follows the launch (image_compression.py:266-269) -
                              * the reduction of the decoder-gradient records then also runs Adam over every listed tensor (below: nic_step_tail);
                              * every other entry point: must be null */
} nic_path_desc;
/* Every crop origin is a multiple of the cell size 1 / step_number (1 when step_number >= 1), e.g. whole-image passes from
 * origin 0: the launch then covers extent / cell blocks per axis instead of the unaligned upper bound extent / cell + 1
 * (origins live on the device, the library cannot look). Setting it for unaligned origins drops samples. */
#define NIC_FLAG_ORIGINS_ALIGNED 1
/* Matrix products on the bf16 matrix pipe with each fp32 operand carried as a hi + lo bf16 pair (16 significant bits, three
 * bf16 MFMAs per product, fp32 accumulation); activations, noise, loss and all accumulators stay fp32.
 *   2D training (nic_fused_forward_backward, _img, nic_fused_backward_dy): every product of the step, 1.8x faster;
 *   3D training: the four chained products (layer 1, layer 2 and their input-gradient transposes), 1.2x faster - the
 *     [sample][feature] bf16 images of the weight-gradient products do not fit the LDS next to the 3D weights;
 *   inference (nic_fused_forward, nic_fused_forward_u8), every layout: layers 1 and 2, 1.6-2x faster.
 * Agreement with the fp32 kernels: outputs ~3e-7, gradients <= 7e-6 relative (the fp32 kernels themselves sit ~1e-6 from the
 * CPU oracle).  The fp32-input MFMA blocks the wave's vector issue, the bf16 one does not. */
#define NIC_FLAG_SPLIT_BF16 2
/* With NIC_FLAG_SPLIT_BF16, 2D training: keep the step on the 4-wave x 32-sample kernel (one wave per SIMD) instead of the default
 * 8-wave x 16-sample kernel (two waves per SIMD; same arithmetic mode, different tiling and summation order).  Kept for
 * comparison runs and as the second implementation the parity tests hold the default against. */
#define NIC_FLAG_SPLIT_TILE32 4
/* With NIC_FLAG_SPLIT_BF16, 2D, n_linear = 3: run the step (or decode) on the depth-generic kernel that serves n_linear = 5 (4 waves per
 * workgroup, the layer loop): the cross-check of that kernel against the dedicated 3-layer kernels. */
#define NIC_FLAG_MLPN 8
/* 16-bit grid STORAGE (the reference's FP_NUM_DTYPE = 16 maps its grids to torch.float16, utils.py:301-313; its own 16-bit run does not
 * train, readme.md:9): g0 / g1 point at bfloat16 or IEEE half arrays of the usual [C, Y, X] shape; every value is widened to fp32 in the
 * gather and all arithmetic, the gradients (dense fp32 tensors of the grids' shapes) and the optimiser state stay fp32 - nic_adam_multi
 * keeps an fp32 master and writes the 16-bit mirror (nic_adam_tensor.param16).  2D with NIC_FLAG_SPLIT_BF16 (nic_fused_forward,
 * nic_fused_forward_backward, _img, nic_fused_backward_dy), or any layout with NIC_FLAG_BF16 (the training entry points). */
#define NIC_FLAG_GRID_BF16 16
#define NIC_FLAG_GRID_FP16 32
/* PLAIN bf16 matrix products (BASELINE.json's "bf16"): every product operand - weights, noisy inputs, GELU outputs,
 * the dZ of every layer, the stored GELU derivatives - is ONE bf16 value, accumulation / biases / activations / loss / grid-gradient
 * sums are fp32 (csrc/fused_q16.hpp lists the rounding points; oracle/nic_oracle.py::mlp_forward_backward_bf16 restates them).
 * Training entry points (nic_fused_forward_backward, _img, nic_fused_backward_dy), every layout (2D, 3D methods 3 and 4),
 * n_linear 3 or 5, fp32 or 16-bit grid storage; 8 waves x 16 samples, two waves per SIMD.  Takes precedence over NIC_FLAG_SPLIT_BF16.
 * Results are checked against the precision-emulating oracle at 1e-3 (outputs) and stay within ~1e-2 of the fp32 arithmetic. */
#define NIC_FLAG_BF16 64
/* PLAIN fp16 matrix products: NIC_FLAG_BF16's kernels, rounding points and entry points with IEEE half operands instead of bfloat16 (the reference's own
 * 16-bit type: FP_NUM_DTYPE / MLP_NUM_DTYPE = 16 map to torch.float16, utils.py:301-313; BASELINE config 3's "fp16"): v_mfma_f32_16x16x32_f16 runs at the
 * bf16 rate with 11 significant bits instead of 8 - outputs ~2e-5 and gradients ~1e-3 from the fp32 arithmetic, checked against the fp32 oracle directly.
 * dZ of a mean over millions of samples is far below the half range (2 loss_scale ~ 1e-7), so the kernel carries 2^k dZ and multiplies every sum of dZ
 * products by 2^-k where it leaves the kernel (exact): k = nic_path_desc.dz_scale_log2, or - 0 - chosen from loss_scale by the MSE entry points.  Default
 * channel counts; takes precedence over NIC_FLAG_BF16 and NIC_FLAG_SPLIT_BF16. */
#define NIC_FLAG_FP16 128
/* The `origins` argument of the FUSED entry points (nic_fused_*) points to HOST memory: num_crops x dim int32 values, num_crops <= NIC_ORIGINS_INLINE_MAX,
 * read during the call and handed to the kernel by value.  The host loop of the reference draws its crop origins on the host
 * (image_compression.py:26-50): a step then needs no upload (a 5 us copy in front of a 0.1 ms kernel) and the kernel no dependent global load in front
 * of its gathers.  Not for the captured loop (nic_fused_forward_backward_img_dev reads the origins nic_sampler_step_begin wrote) nor for the
 * layer-wise entry points (nic_encode*, nic_gather_corners, ..: NIC_E_ARG). */
#define NIC_FLAG_ORIGINS_HOST 256
#define NIC_ORIGINS_INLINE_MAX 16

/* ColorDecoder parameters (image_compression.py:54-68): state_dict keys decoder.{0,2,4}.{weight,bias}.  The reference hard-codes 3
 * Linear layers (n_linear = 3, or 0); n_linear = 5 is the "4 x 64" decoder of BASELINE.json's north star - Linear(Cin,H), three
 * Linear(H,H), Linear(H,3), GELU between, Sigmoid at the end (keys decoder.{0,2,4,6,8}) - supported by the fused 2D entry points with
 * NIC_FLAG_SPLIT_BF16 (nic_fused_forward, nic_fused_forward_backward, _img, nic_fused_backward_dy); everything else returns
 * NIC_E_UNSUPPORTED for it.  Layer i lives in w[i] / b[i]; the output layer is the last one. */
#define NIC_MAX_LINEAR 5
typedef struct nic_mlp {
    const float *w[NIC_MAX_LINEAR]; /* [H,Cin], [H,H] x (n_linear - 2), [3,H] */
    const float *b[NIC_MAX_LINEAR]; /* [H], [H] x (n_linear - 2), [3] */
    int32_t n_linear;               /* 3 (0 means 3) or 5; nic_decoder_general_*: 2 .. NIC_MAX_LINEAR */
    int32_t reserved;
} nic_mlp;

typedef struct nic_mlp_grads {
    float *w[NIC_MAX_LINEAR];
    float *b[NIC_MAX_LINEAR];
} nic_mlp_grads;

int nic_abi_version(void);
const char *nic_error_string(int code);

/* Number of decoder input channels Cin (var2.py:114-118). */
int nic_decoder_input_channels(int dim, int method, int channels, int pe_channels);

/* Bytes of scratch the *_backward entry points need (per-wave partial sums of the decoder gradients,
 * reduced in a fixed order by a second kernel so decoder gradients and loss are run-to-run bit-stable). */
size_t nic_workspace_bytes(const nic_path_desc *desc);

/* ---- encode only: replaces create_decoder_input_2d/_3d/_3d_v2 and finally_decode_input_*
 *      (image_compression.py:71-211).  out = [N, Cin].  origins = int32 [num_crops, dim]. */
int nic_encode(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
               float *out, void *stream);

/* ---- autograd backward of nic_encode: dx = [N, Cin] -> scatter-add into g0_grad / g1_grad (shapes of g0 / g1, NOT
 *      zeroed here: fp32 atomic adds, the reference's index_put_(accumulate=True) from loss.backward(),
 *      image_compression.py:265).  The PE and LOD columns of dx have no parameters behind them and are ignored. */
int nic_encode_backward(const nic_path_desc *desc, const int32_t *origins, const float *dx, float *g0_grad,
                        float *g1_grad, void *stream);

/* ---- encode, split outputs: replaces create_g0_g1 / _3d / _3d_v2 (fp_def.py:115-223) for ONE crop.
 *      out = [K0*C + K1*C + P*dim, n] rows: raw G0 corners, weighted G1 corners (not summed), PE. */
int nic_encode_split(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                     float *out, void *stream);

/* ---- corner gathers on explicit index vectors: replaces create_g / create_g_3d / create_g_3d_v2 (fp_def.py:81-112).
 *      grid = [C, (nz,) ny, nx]; xi / yi / zi = int32 [n] (zi null in 2D); corner_set 0: the 4 corners of 2D,
 *      1: the 8 corners of 3D, 2: the 4 tetrahedral corners; out = [K, C, n] in the reference's corner order.
 *      Indices are clamped into the grid (the reference would raise IndexError). */
int nic_gather_corners(const float *grid, int channels, int nx, int ny, int nz, const int32_t *xi, const int32_t *yi,
                       const int32_t *zi, int64_t n, int corner_set, float *out, void *stream);

/* ---- positional encodings on explicit coordinates (utils.py:198-227).  coord = [dim, n], out = [P*dim, n]. */
int nic_positional_encoding(const float *coord, int64_t n, int dim, int pe_channels, int pe_mode,
                            const float *pe_div_host, float *out, void *stream);

/* ---- LUT positional encoding gather: replaces TriangularPositionalEncoding1D.forward
 *      (positional_encoding.py:36-42).  lut = [rows, seq_len], coord = int64 [b, L], out = [b, rows, L]. */
int nic_lut_gather(const float *lut, int rows, int seq_len, const int64_t *coord, int64_t b, int64_t L,
                   float *out, void *stream);

/* ---- decoder on explicit inputs: replaces ColorDecoder.forward (image_compression.py:66-68).
 *      x = [n, cin], y = [n, 3]. */
int nic_decoder_forward(const nic_mlp *mlp, const float *x, int64_t n, int cin, int hidden, float *y, void *stream);

/* ---- its autograd backward: dy = [n,3] -> dx = [n,cin] (may be null) and the six parameter gradients
 *      (overwritten, not accumulated). */
int nic_decoder_backward(const nic_mlp *mlp, const float *x, const float *dy, int64_t n, int cin, int hidden,
                         float *dx, const nic_mlp_grads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the same decoder for ANY Cin >= 1, HIDDEN_LAYER_CHANNELS >= 1 (var2.py:72) and 2 <= n_linear <= NIC_MAX_LINEAR, on explicit
 *      inputs: layer-wise LDS-tiled fp32 products (csrc/decoder_general.hip), the route of every flag combination the fused kernels do
 *      not specialise (ColorDecoder.forward, image_compression.py:54-68, with HIDDEN_LAYER_CHANNELS / FEATURE_PYRAMID_CHANNELS /
 *      PE_CHANNELS of any value).  The sample axis is walked in chunks; the workspace (nic_decoder_general_workspace_bytes for the same
 *      n, cin, hidden, n_linear; training = 1 for the backward call) holds one chunk's activations, their GELU derivatives and the
 *      per-slice weight-gradient sums.  _backward recomputes the forward pass of a chunk itself: x and dy in, dx (may be null) and the
 *      2 n_linear parameter gradients out (overwritten; null entries are skipped; fixed summation order, bit-stable run to run). */
size_t nic_decoder_general_workspace_bytes(int64_t n, int cin, int hidden, int n_linear, int training);
int nic_decoder_general_forward(const nic_mlp *mlp, const float *x, int64_t n, int cin, int hidden, float *y, void *workspace,
                                size_t workspace_bytes, void *stream);
int nic_decoder_general_backward(const nic_mlp *mlp, const float *x, const float *dy, int64_t n, int cin, int hidden, float *dx,
                                 const nic_mlp_grads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- HIDDEN_LAYER_CHANNELS below 64 on the FUSED kernels (which are built for 64): a decoder with H hidden units IS the decoder with 64 units
 *      whose extra units have zero weights and biases (pre-activation 0, GELU(0) = 0, zero outgoing weights: exact zero gradients).
 *      nic_decoder_pad writes the zero-padded copies ([H, K] -> [hidden_padded, K'], the output layer [3, H] -> [3, hidden_padded]) into the
 *      caller's `dst` tensors, the fused entry points run on them with desc->hidden = hidden_padded, nic_decoder_unpad copies the real block of
 *      every padded gradient into the caller's gradient tensors (null entries of `dst` are skipped).  One launch each; fused.PaddedMlp does this
 *      for every fused entry point of the Python side. */
int nic_decoder_pad(const nic_mlp *src, int cin, int hidden, int hidden_padded, const nic_mlp_grads *dst, void *stream);
int nic_decoder_unpad(const nic_mlp_grads *src_padded, int n_linear, int cin, int hidden, int hidden_padded, const nic_mlp_grads *dst,
                      void *stream);

/* ---- fused inference: encode + (optional noise) + decoder.  Replaces finally_decode_input_* + arc_decoder(x)
 *      inside decode_image (image_compression.py:313-345).  y = [N, 3]. */
int nic_fused_forward(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                      const nic_mlp *mlp, const float *noise, float *y, void *stream);

/* ---- the same training step with the target read straight from a resident image instead of an [N,3] tensor (SURVEY 8f
 *      rank 3; the sampler's slicing / reshape / stack of image_compression.py:37-47 disappears): sample i of crop k takes
 *      image[c][origin_k + i].  `data` is the reference's dataset tensor [3, S0, S1(, S2)] (first spatial axis = first sample
 *      axis), contiguous, fp32 - or uint8 codes with target = u / den, correctly rounded like torch's true division (den 255:
 *      ToTensor, image_compression.py:436-440; den 256: the 3D loader, :474).  Every origin + extent must lie inside `size`. */
typedef struct nic_target_image {
    const void *data;
    int32_t is_u8;       /* 0: fp32 planar [3, S0, S1(, S2)].  1: uint8 planar, target = u / den.  2: uint8 RGBX interleaved
                          *    [S0, S1(, S2)] dwords R | G << 8 | B << 16 (nic_rgbx_interleave / nic_rgbx_downsample2): the three
                          *    targets of a sample are ONE load, target = byte / den */
    float den;           /* uint8 only */
    int32_t size[3];     /* S0, S1, S2 (1 for 2D) */
    int32_t reserved;
} nic_target_image;
int nic_fused_forward_backward_img(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                                   const nic_mlp *mlp, const float *noise, const nic_target_image *image, float *y, float *loss,
                                   float *g0_grad, float *g1_grad, const nic_mlp_grads *grads, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ---- device-side sampler (image_compression.py:26-50, 221-226).  The reference draws the LOD with Python's
 *      `random` and the crop origins with torch.randint on the host and uploads them every step; this counter-based generator
 *      (Threefry-4x32-12 keyed by seed, step and crop; csrc/nic_device.hpp::sampler_block) gives the same LAWS - LOD uniform on
 *      0..max_mip, or floor(-log2 U / 2) = clz(word) >> 1; origins uniform on [0, range) per axis - without host RNG state:
 *      the LOD decides the launch geometry, so it is evaluated on the host (pure function, no GPU); the origins are written by a
 *      tiny kernel straight into the int32 [num_crops, dim] device buffer the fused entry points read - no upload per step.
 *      nic_sampler_origins_host is the same function on the host (tests, debugging). */
int nic_sampler_lod_host(uint64_t seed, uint64_t step, int uniform_distribution, int max_mip_level);
int nic_sampler_origins_host(uint64_t seed, uint64_t step, int num_crops, int dim, int32_t range, int32_t *origins_host);
int nic_sampler_draw_origins(uint64_t seed, uint64_t step, int num_crops, int dim, int32_t range, int32_t *origins, void *stream);

/* ---- resident RGBX target images: planar uint8 [3][n] (the codes ToTensor / the 3D loader divide, image_compression.py:436-440, 474)
 *      -> n dwords; and the next level of a 2D mip chain by a 2 x 2 box filter with round-to-nearest (the reference resizes with
 *      torchvision's Resize, :429-477: its filter is not reproduced - targets at mip > 0 are this library's own definition;
 *      mip 0, the only level of the no-mip default, is exact). */
int nic_rgbx_interleave(const uint8_t *planar, int64_t n, uint32_t *rgbx, void *stream);
int nic_rgbx_downsample2(const uint32_t *src_rgbx, int s0, int s1, uint32_t *dst_rgbx, void *stream);
/* ---- the reference's OWN mip filter: transforms.Resize on the PIL image (image_compression.py:434-440) is Pillow's two-pass fixed-point resize
 *      (src/libImaging/Resample.c; torchvision is a thin wrapper: functional.resize -> Image.resize(size, BILINEAR)).  One pass along `axis` of an RGBX
 *      image [s0][s1] (axis 1 = the contiguous one; Pillow runs it first, then axis 0): out = clip8((2^21 + sum_t pixel[lo + t] * kk[o][t]) >> 22) per
 *      channel, taps [lo, lo + count) = bounds[o][0..1], kk int32 [out_size][ksize] in 2^-22 units - precompute_coeffs + normalize_coeffs_8bpc, restated
 *      on the host by sampler.resize_coeffs.  Every level is resized from the ORIGINAL image, like the reference.  Bit-exact against Pillow
 *      (tests/test_host_cpu.py pins the coefficients, tests/test_gpu_general.py the images). */
int nic_rgbx_resample_axis(const uint32_t *src_rgbx, int s0, int s1, int axis, int out_size, const int32_t *bounds, const int32_t *kk, int ksize,
                           uint32_t *dst_rgbx, void *stream);

/* ---- decode straight from the stored codec (image_compression.py:307-346 after fp_load, fp_def.py:258-263):
 *      the grids are the uint8 tensors fp_savable wrote (models.py:61-64), dequantised in-kernel exactly like load4fp
 *      (models.py:68-71), so the result is bit-identical to nic_load4fp_u8 + nic_fused_forward at a quarter of the grid bytes.
 *      desc->num_bits is the codec's bit depth (1..8); desc->noise_mode must be NIC_NOISE_NONE.  n_linear 3: every layout; n_linear 5: 2D
 *      (split-bf16 products, like nic_fused_forward for that depth).
 *      y: fp32 [N,3] and/or y_u8: quantize_to_bit(y) as bytes (models.py:39-40) - at least one. */
int nic_fused_forward_u8(const nic_path_desc *desc, const uint8_t *g0_u8, const uint8_t *g1_u8, const int32_t *origins,
                         const nic_mlp *mlp, float *y, uint8_t *y_u8, void *stream);

/* ---- fused training step core: encode + noise + decoder + MSE loss + full backward.  Replaces
 *      image_compression.py:239-265 (create_decoder_input_*, rand_like noise, decoder(...), MSELoss, backward).
 *      target = [N,3].  y may be null.  loss = 1 float (the mean, desc->loss_scale * sum of squared error).
 *      g0_grad / g1_grad have the shapes of g0 / g1 and must be ZEROED by the caller (the kernel adds into
 *      them with fp32 atomics, like index_put_(accumulate=True)); decoder gradients and loss are overwritten. */
int nic_fused_forward_backward(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                               const nic_mlp *mlp, const float *noise, const float *target, float *y, float *loss,
                               float *g0_grad, float *g1_grad, const nic_mlp_grads *grads,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---- same, for an arbitrary upstream gradient dy = [N,3] instead of the built-in MSE (autograd backward of
 *      nic_fused_forward; the forward is recomputed). */
int nic_fused_backward_dy(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                          const nic_mlp *mlp, const float *noise, const float *dy,
                          float *g0_grad, float *g1_grad, const nic_mlp_grads *grads,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- quantisers / codec (models.py:55-71, fp_def.py:227-263).  In-place allowed (dst == src). */
int nic_quantize(const float *src, float *dst, int64_t n, int num_bits, void *stream);              /* floor(x*(2^b-1)+.5)/(2^b-1) */
int nic_quantize_to_bit(const float *src, float *dst, int64_t n, int num_bits, void *stream);       /* models.py:39-40 */
int nic_clamp(float *x, int64_t n, float lo, float hi, void *stream);                                /* fp_quantize_clamp */
int nic_save4fp_u8(const float *src, uint8_t *dst, int64_t n, int num_bits, void *stream);          /* models.py:61-64 */
int nic_load4fp_u8(const uint8_t *src, float *dst, int64_t n, int num_bits, void *stream);          /* models.py:68-71 */

/* ---- PSNR with peak = 2^num_bits (utils.py:117-130): out[0] = mse, out[1] = psnr dB (inf when mse == 0). */
int nic_psnr(const float *a, const float *b, int64_t n, int num_bits, float *out2, void *workspace, size_t workspace_bytes, void *stream);

/* ---- fused Adam step + in-place clamp for one parameter tensor (image_compression.py:266-269, 361-365):
 *      torch.optim.Adam semantics (no weight decay, no amsgrad), bias-corrected with step count `step` (1-based).
 *      clamp_lo > clamp_hi disables the clamp.  The hyper-parameters are doubles because torch's are Python floats: the library
 *      forms (float)(1 - beta), (float)(lr / bias_correction1) exactly as torch does (1.0f - 0.999f != 0.001f).  The clamp keeps
 *      NaN (torch.clamp_ propagates it; a diverged grid must not be silently reset to clamp_lo). */
int nic_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, int64_t step, float clamp_lo, float clamp_hi, void *stream);

/* ---- the whole optimiser step in ONE launch: Adam for every listed tensor - grids at lr 0.01, decoder
 *      at lr 0.005, each already scaled by the caller's CosineAnnealingLR factor - with the fp_quantize_clamp of the grids
 *      folded in (image_compression.py:266-269, 361-365; fp_def.py:227-232).  torch keeps one step counter per parameter
 *      (a parameter whose .grad is None is skipped and does not advance), hence `step` per tensor.  The tensor table is
 *      read on the host and passed to the kernel by value: at most NIC_ADAM_MAX_TENSORS per call. */
#define NIC_ADAM_MAX_TENSORS 32
typedef struct nic_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;
    int64_t step;            /* 1-based step count of THIS tensor */
    double lr;
    float clamp_lo, clamp_hi; /* clamp_lo > clamp_hi: no clamp */
    void *param16;            /* null, or a 16-bit mirror of `param` (same element count) rewritten with the rounded new values */
    int32_t param16_kind;     /* 1: bfloat16, 2: IEEE half (round to nearest even) */
    int32_t flags;            /* NIC_ADAM_ZERO_GRAD: the launch also zeroes `grad` (written through the const pointer) once it has been read - the
                                 gradient bucket of an atomically accumulating step is clean for the next step without a fill kernel; 0 otherwise */
    int32_t reps;             /* 0 / 1: one contiguous run of n elements.  r > 1: r runs of n elements each - run k starts k * rep_stride elements into
                                 param / grad / param16 and k * state_rep_stride into exp_avg / exp_avg_sq: a block of node rows of EVERY channel of a
                                 grid [C, rows, ..] in one entry (rep_stride = the channel plane) with moments allocated for those rows only
                                 (state_rep_stride = n) - the stripe-owned optimiser of the multi-GPU step */
    int32_t reserved;
    int64_t rep_stride, state_rep_stride;
} nic_adam_tensor;
#define NIC_ADAM_ZERO_GRAD 1
#define NIC_ADAM_SCHED_COL1 2 /* nic_adam_multi_dev: this tensor takes its step size from column 1 of the schedule (the decoder group), else column 0 */
int nic_adam_multi(const nic_adam_tensor *tensors, int count, double beta1, double beta2, double eps, void *stream);

/* ---- the optimiser step as the TAIL of the fused training step (nic_path_desc.tail): image_compression.py:263-269 (backward, optimizer.step,
 *      fp_quantize_clamp) in TWO launches instead of three or four.  A training entry point ends with the reduction of the per-workgroup
 *      decoder-gradient records; with a tail that launch gets more blocks: the first `n_stream` tensors (the grids: their gradients are complete
 *      when the fused kernel ends) are streamed by the extra blocks exactly as nic_adam_multi would - NIC_ADAM_ZERO_GRAD, clamp and 16-bit
 *      mirror included - WHILE the reduction walks the records (it is latency-bound, the streaming HBM-bound); the remaining tensors are the
 *      decoder's: their .grad must be the nic_mlp_grads buffers of the same call, and the thread that finishes element i of such a gradient
 *      updates parameter i on the spot.  Same arithmetic as nic_adam_multi after the plain entry point, bit for bit.  count <= NIC_ADAM_MAX_TENSORS;
 *      sched / sched_rows: nic_adam_multi_dev's device schedule, read with the `step_dev` of nic_fused_forward_backward_img_dev (null: the
 *      per-tensor .step / .lr are used). */
/* measurement hook (bench.py's roofline leg): the NEXT training entry point called on this thread records `hip_event` (a hipEvent_t) on its
 * stream right after its fused kernel - before the reduction / tail launch - so that HIP events can bracket the dominant kernel alone inside
 * a timed region of whole steps.  One-shot; null clears it. */
int nic_mark_kernel_end(void *hip_event);

typedef struct nic_step_tail {
    const nic_adam_tensor *tensors;
    int32_t count;
    int32_t n_stream;
    double beta1, beta2, eps;
    const float *sched;
    int64_t sched_rows;
} nic_step_tail;

/* ---- hipGraph-captured training loops (no reference counterpart: the reference's loop is host Python, image_compression.py:215-303).
 *      The reference's own launchers run 320 000 steps of 8 x 32^3 samples: the GPU needs ~0.1 ms per step, the host loop twice that.
 *      With the step number in DEVICE memory one captured sequence [nic_sampler_step_begin -> nic_fused_forward_backward_img_dev ->
 *      nic_adam_multi_dev] serves every step and is replayed without the host touching a single argument:
 *        counters   int64 [2] device: [0] = next step to run, [1] = the step in flight (what the other two entry points read through
 *                   `step_dev` = counters + 1)
 *        nic_sampler_step_begin  t = counters[0]; counters[1] = t; counters[0] = t + 1; loss_hist[t - 1] = *loss_slot (the loss the previous
 *                   step's reduction wrote; either pointer may be null); origins of step t as nic_sampler_draw_origins(seed, t, ..)
 *        nic_fused_forward_backward_img_dev  nic_fused_forward_backward_img with noise offset desc->noise_offset + *step_dev (in-kernel noise
 *                   or none; kernels: 2D NIC_FLAG_SPLIT_BF16 with 3 layers, or NIC_FLAG_BF16 - otherwise NIC_E_UNSUPPORTED)
 *        nic_adam_multi_dev  nic_adam_multi with the per-step scalars read from row min(*step_dev, sched_rows - 1) of `sched`, a device
 *                   table [sched_rows][4] of floats the caller fills once: {lr_0 / bias_correction1, lr_1 / bias_correction1,
 *                   sqrt(bias_correction2), 0} for Adam step row + 1 (formed in double and cast once, like nic_adam_multi does per call);
 *                   nic_adam_tensor.step / .lr are ignored, NIC_ADAM_SCHED_COL1 selects the column. */
int nic_sampler_step_begin(uint64_t seed, int64_t *counters, int num_crops, int dim, int32_t range, int32_t *origins,
                           const float *loss_slot, float *loss_hist, int64_t hist_len, void *stream);
int nic_fused_forward_backward_img_dev(const nic_path_desc *desc, const float *g0, const float *g1, const int32_t *origins,
                                       const nic_mlp *mlp, const nic_target_image *image, float *loss, float *g0_grad, float *g1_grad,
                                       const nic_mlp_grads *grads, const int64_t *step_dev, void *workspace, size_t workspace_bytes,
                                       void *stream);
int nic_adam_multi_dev(const nic_adam_tensor *tensors, int count, double beta1, double beta2, double eps, const float *sched,
                       int64_t sched_rows, const int64_t *step_dev, void *stream);

/* ---- MULTI-LEVEL fused step (no reference semantics: the reference reads ONE level pair per sample, fp_def.py:24-34, image_compression.py:76-79;
 *      BASELINE.json config 2 names a "16-level grid", SURVEY 0 asks for the level count as a kernel parameter).  A sample gathers from the first
 *      `levels` level pairs AT ONCE and the decoder sees their encodings concatenated:
 *          x = [enc_0 | .. | enc_{levels-1} | lod],  enc_l = [G0_l corners (4 C) | blended G1_l (C) | PE_l (2 P)]
 *      enc_l being exactly what create_g0_g1 (fp_def.py:115-145) computes for pair l at step_number 2^(desc->log2_step - 2 l) (image_compression.py:79:
 *      4^-(l+1) at mip 0), the positional encoding on THAT pair's G1-cell coordinate; Cin = levels (5 C + 2 P) + 1 (decoder weights mlp->w[0] = [H, Cin]).
 *      2D (desc->dim = 2, method = 1), fp32 grids, plain-bf16 products (the arithmetic of NIC_FLAG_BF16: csrc/fused_q16.hpp), in-kernel / tensor / no
 *      noise, ONE launch: gathers, noise, decoder forward, loss, backward, one atomic flush per touched cell and pair.  Fused kernels exist for
 *      (levels, C, n_linear) in {(2,4,3), (3,4,3), (5,4,3), (2,4,5), (3,4,5), (2,12,3), (3,12,3)} with P = 6, H = 64 (what fits the 160 KB of LDS beside the
 *      [64, Cin] weight image); everything else returns NIC_E_UNSUPPORTED (the caller composes nic_encode x levels + the general decoder instead).
 *      desc->g0_nodes / g1_nodes are ignored (pairs carry their own); desc->extent, num_crops, origins, noise, loss_scale, sample_base as in
 *      nic_fused_forward_backward.  Gradients are ADDED into pairs->g0_grad / g1_grad (dense fp32 tensors of the grids' shapes, zeroed by the caller). */
#define NIC_ML_MAX_LEVELS 5
typedef struct nic_ml_pairs {
    int32_t levels;                               /* 2 .. NIC_ML_MAX_LEVELS */
    int32_t reserved;
    const float *g0[NIC_ML_MAX_LEVELS];           /* [C, ny, nx] fp32 */
    const float *g1[NIC_ML_MAX_LEVELS];
    float *g0_grad[NIC_ML_MAX_LEVELS];            /* training entry point only */
    float *g1_grad[NIC_ML_MAX_LEVELS];
    int32_t g0_nodes[NIC_ML_MAX_LEVELS][2];       /* nodes per axis (x, y) */
    int32_t g1_nodes[NIC_ML_MAX_LEVELS][2];
} nic_ml_pairs;
int nic_fused_ml_forward_backward(const nic_path_desc *desc, const nic_ml_pairs *pairs, const int32_t *origins, const nic_mlp *mlp,
                                  const float *noise, const float *target, float *y, float *loss, const nic_mlp_grads *grads,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* forward only (decode): y = [N, 3] */
int nic_fused_ml_forward(const nic_path_desc *desc, const nic_ml_pairs *pairs, const int32_t *origins, const nic_mlp *mlp, float *y,
                         void *stream);

/* ---- multi-GPU, stripe-sharded grids (no reference counterpart - the reference is single-device): the per-step exchange buffer
 *      [small | boundary rows of G0 | boundary rows of G1].  `small` = the head of the flat gradient bucket (loss + decoder gradients,
 *      n_small floats); a row set = `nrows` node rows (hyper-planes of the slowest spatial axis: `row_elems` contiguous floats) of every one of
 *      `channels` channel planes (`plane` floats apart) of one grid-gradient tensor.  nic_stripe_pack gathers everything into `buf`
 *      (layout: small, then per set [channel][row][row_elems]); the caller all-reduces `buf` over RCCL; nic_stripe_unpack writes the sums
 *      back.  One launch each (the torch formulation was index_select x 2 + cat + copy + index_copy x 2 per step). */
#define NIC_STRIPE_MAX_ROWS 15
typedef struct nic_row_set {
    float *base;             /* the gradient tensor [C, rows, row_elems...] */
    int64_t plane;           /* floats per channel */
    int32_t row_elems;       /* floats per node row */
    int32_t channels;
    int32_t nrows;           /* <= NIC_STRIPE_MAX_ROWS */
    int32_t rows[NIC_STRIPE_MAX_ROWS];
} nic_row_set;
int nic_stripe_pack(const float *small_buf, int64_t n_small, const nic_row_set *sets, int nsets, float *buf, void *stream);
int nic_stripe_unpack(float *small_buf, int64_t n_small, const nic_row_set *sets, int nsets, const float *buf, void *stream);

/* ---- multi-resolution hash-grid encoding (no reference counterpart: an Instant-NGP-style extension, neural_image_compression_v2_amd/hashgrid.py).
 *      A field covers integer sample coordinates i_a in [0, S_a) on `dim` axes, S_max = max_a S_a.  Level l has resolution R_l (host-computed) and
 *      a table of T = 2^log2_table entries of `features` floats: table = [levels, T, features] fp32.  On axis a, q = (2 i_a + 1) R_l:
 *      base vertex v_a = floor(q / (2 S_max)) (exact integer), weight w_a = (q mod 2 S_max) / (2 S_max) (fp32).  Entry of vertex v:
 *      (R_l + 1)^dim <= T: v_x + (R_l + 1) (v_y + (R_l + 1) v_z); otherwise (v_x * 1) ^ (v_y * 2654435761u) ^ (v_z * 805459861u) in wrapping uint32;
 *      both & (T - 1).  out = [N, levels * features]: column l F + f = sum over the 2^dim corners c of prod_a (c_a ? w_a : 1 - w_a) table[l, idx(v + c), f].
 *      Samples: crops back to back, x-outer .. last axis inner (like nic_encode); origins = [num_crops, dim] int32 (device).
 *      nic_hash_encode_backward ADDS dx = d loss / d out into table_grad (fp32 atomics; the caller zeroes it); summation order is not fixed. */
#define NIC_HASH_MAX_LEVELS 32
typedef struct nic_hash_desc {
    int32_t dim;             /* 2 or 3 */
    int32_t levels;          /* 1 .. NIC_HASH_MAX_LEVELS */
    int32_t features;        /* 1, 2, 4 or 8 */
    int32_t log2_table;      /* 10 .. 24 */
    int32_t S_max;           /* largest field extent; 2 S_max R_l < 2^31 */
    int32_t num_crops;
    int32_t extent[3];       /* samples per axis of one crop; extent[2] = 1 in 2D */
    int32_t resolution[NIC_HASH_MAX_LEVELS];   /* R_l >= 1 */
    int32_t flags;           /* 0 */
    int32_t reserved;
} nic_hash_desc;
int nic_hash_encode(const nic_hash_desc *desc, const float *table, const int32_t *origins, float *out, void *stream);
int nic_hash_encode_backward(const nic_hash_desc *desc, const int32_t *origins, const float *dx, float *table_grad, void *stream);
/* the entry index of vertex (vx, vy, vz) at `level` (vz = 0 in 2D) from the same function the kernels use, or a NIC_E_* code */
int nic_hash_index_host(const nic_hash_desc *desc, int level, int32_t vx, int32_t vy, int32_t vz);

/* ---- hash-grid codec: quantisation-aware training and a uint8 stored table (hashgrid.py, HashGridField(num_bits=b)).
 *      Bits b in 1..8; the table is clamped to the dense quantiser's range [-(2^b - 1) / 2^(b+1), 1/2] (models.py:48-51) by the optimiser.
 *      nic_hash_encode_noisy: out = fl(nic_hash_encode out + noise), noise on EVERY column (the reference's rand_like on the decoder input,
 *      image_compression.py:250, amplitude 2^-b).  Sample id s = sample_base + n (n = the row of the launch); column c = l F + f is value
 *      c & 15 of generator block c >> 4: Threefry-4x32-12 of counter (s_lo, (c >> 4) + (s_hi << 8), offset_lo, offset_hi), key (seed_lo,
 *      seed_hi, "NIC2", 0); value i = byte i & 3 of word i >> 2, u8 -> ((u8 + 1/2) / 256 - 1/2) 2^-b (nic_device.hpp::noise_from_block).
 *      Straight-through backward: nic_hash_encode_backward serves both forms.
 *      Compact stored table (uint8): levels back to back, level l holds E_l = min((R_l + 1)^dim, T) entries of `features` bytes in entry order
 *      (a dense level: exactly the vertices it can address; a hashed one: all T), starting at byte F * sum_{k<l} E_k.  Byte = save4fp
 *      (nic_save4fp_u8: floor(x (2^b - 1) + 1/2) + 2^(b-1) - 1, truncated to uint8); nic_hash_encode_u8 dequantises each corner with
 *      nic_load4fp_u8's arithmetic ((u - 2^(b-1) + 1) / (2^b - 1)) and then blends exactly like nic_hash_encode: its output equals
 *      nic_hash_encode of load4fp(save4fp(table)) bit for bit.  nic_hash_pack_u8 writes the compact table from the fp32 [L, T, F] one
 *      (the caller clamps first: an out-of-range value wraps in the uint8 cast, like the dense codec).  Every argument error is returned
 *      on the host before any GPU work; a nonzero desc->flags stays NIC_E_ARG. */
typedef struct nic_hash_quant {
    int32_t num_bits;        /* 1 .. 8 */
    int32_t noise_mode;      /* NIC_NOISE_NONE or NIC_NOISE_KERNEL (NIC_NOISE_TENSOR: NIC_E_UNSUPPORTED) */
    uint64_t noise_seed;
    uint64_t noise_offset;   /* e.g. the optimiser step */
    int64_t sample_base;     /* global id of this launch's row 0 (>= 0) */
} nic_hash_quant;
int nic_hash_encode_noisy(const nic_hash_desc *desc, const nic_hash_quant *quant, const float *table, const int32_t *origins, float *out,
                          void *stream);
int nic_hash_encode_u8(const nic_hash_desc *desc, int num_bits, const uint8_t *stored, const int32_t *origins, float *out, void *stream);
int nic_hash_pack_u8(const nic_hash_desc *desc, int num_bits, const float *table, uint8_t *stored, void *stream);   /* [L, T, F] fp32 -> compact */
int64_t nic_hash_stored_bytes(const nic_hash_desc *desc);   /* F * sum_l E_l, or a negative NIC_E_* code */

/* ---- hash-grid codec: the bit-packed stored table, b bits per value (hashgrid.py, save_compressed(packed=True)).
 *      With E_l as above and u the byte nic_hash_pack_u8 writes for a table value (0 <= u <= 2^b - 1 inside the clamp range):
 *      level l is a little-endian bit stream; value f of entry e occupies bits [(e F + f) b, (e F + f + 1) b), least significant bit first;
 *      bit k of the stream is bit k & 7 of byte k >> 3; the stored value is u & (2^b - 1).  Each level's stream is padded with zero bits to a
 *      multiple of 4 bytes, so level l starts at byte 4 sum_{k<l} ceil(E_k F b / 32).  After the last level come 8 zero bytes: a gather reads a
 *      window of up to three aligned dwords from the dword an entry starts in (F b <= 64, start bit <= 31) and never leaves the buffer.
 *      nic_hash_packed_bytes = 4 sum_l ceil(E_l F b / 32) + 8 (or a negative NIC_E_* code); at b = 8 each level's bytes are the uint8 format's.
 *      nic_hash_pack_bits writes the whole buffer from the fp32 [L, T, F] table (padding and tail as zeros; nic_hash_pack_u8's arithmetic per
 *      value), nic_hash_unpack_bits turns it back into the compact uint8 table, nic_hash_encode_bits is nic_hash_encode_u8 from the packed
 *      table, bit for bit (the masked value takes the same dequantisation and blend).  `packed` must be 4-byte aligned (else NIC_E_ARG, after
 *      the checks the _u8 siblings make, which come in the same order with the same codes, all before any GPU work). */
int64_t nic_hash_packed_bytes(const nic_hash_desc *desc, int num_bits);
int nic_hash_pack_bits(const nic_hash_desc *desc, int num_bits, const float *table, uint8_t *packed, void *stream);
int nic_hash_unpack_bits(const nic_hash_desc *desc, int num_bits, const uint8_t *packed, uint8_t *stored, void *stream);
int nic_hash_encode_bits(const nic_hash_desc *desc, int num_bits, const uint8_t *packed, const int32_t *origins, float *out, void *stream);

/* ---- hash-grid encoding + decoder in ONE kernel (hashgrid.py, HashGridField(fused=True)).  Nothing new is computed: the
 *      encoding is nic_hash_encode's (nic_hash_encode_noisy's with `quant`, nic_hash_encode_u8's from the compact table), the decoder is
 *      ColorDecoder(levels * features, 64, 3) with the GELU / sigmoid of the other kernels in fp32 MFMA arithmetic, the loss is
 *      mean((y - target)^2) * loss_scale over the [N, 3] outputs of the launch, the backward is straight-through into the table - but the
 *      [N, L F] row and its gradient stay on the chip.  Supported: dim 2 / 3, features 1 / 2 / 4 / 8, levels * features <= 64, hidden 64,
 *      3 Linear layers (mlp->n_linear 3 or 0); everything else is NIC_E_UNSUPPORTED, and every argument error is returned on the host before any
 *      GPU work.  nic_hash_fused_supported answers for a (desc, hidden, n_linear) without pointers: NIC_OK or the code the entry points return.
 *      nic_hash_fused_forward_backward: two launches, the fused kernel and the fixed-order reduction of its per-workgroup decoder-gradient
 *      records (workspace >= nic_hash_fused_workspace_bytes, else NIC_E_WORKSPACE).  table_grad: d loss / d table is ADDED with fp32 atomics
 *      (the caller zeroes it; order not fixed); null = frozen table, no scatter.  quant: null or noise_mode NIC_NOISE_NONE = no noise.
 *      flags: NIC_HASH_FUSED_ADD_GRADS - the decoder gradients are added to what mlp_grads holds (the later chunks of a chunked pass), else
 *      overwritten; NIC_HASH_FUSED_ADD_LOSS - the same for *loss.  y: null or [N, 3].  tail: null, or the optimiser step riding on the
 *      reduction exactly as nic_path_desc.tail does (the first n_stream tensors streamed - the table -, the rest the decoder's, their .grad
 *      the mlp_grads buffers of this call, else NIC_E_ARG; no device schedule).  Honours nic_mark_kernel_end like every training entry point. */
#define NIC_HASH_FUSED_ADD_GRADS 1
#define NIC_HASH_FUSED_ADD_LOSS 2
int nic_hash_fused_supported(const nic_hash_desc *desc, int hidden, int n_linear);
size_t nic_hash_fused_workspace_bytes(const nic_hash_desc *desc, const nic_mlp *mlp);   /* 0: unsupported */
int nic_hash_fused_forward(const nic_hash_desc *desc, const float *table, const int32_t *origins, const nic_mlp *mlp, float *y, void *stream);
int nic_hash_fused_forward_u8(const nic_hash_desc *desc, int num_bits, const uint8_t *stored, const int32_t *origins, const nic_mlp *mlp,
                              float *y, void *stream);
/* nic_hash_fused_forward_u8 from the bit-packed table (format above; `packed` 4-byte aligned); nic_hash_fused_supported answers for it too */
int nic_hash_fused_forward_bits(const nic_hash_desc *desc, int num_bits, const uint8_t *packed, const int32_t *origins, const nic_mlp *mlp,
                                float *y, void *stream);
int nic_hash_fused_forward_backward(const nic_hash_desc *desc, const nic_hash_quant *quant, const float *table, const int32_t *origins,
                                    const nic_mlp *mlp, const float *target, float loss_scale, float *table_grad,
                                    const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags, void *workspace, size_t workspace_bytes,
                                    const nic_step_tail *tail, void *stream);

/* ---- the hash-grid field at arbitrary points (hashgrid.py, HashGridField.query / resample / train_points).
 *      A point is `dim` fp32 coordinates in SAMPLE UNITS: p_a = i is the centre of integer sample i, the field spans [-1/2, S_a - 1/2].
 *      points = [n_points, dim] fp32 (device; the host never reads it), row n of every output belongs to point n, in any order.
 *      For these entry points desc->extent[a] is the field size S_a and desc->num_crops must be 1 (else NIC_E_SHAPE).
 *      Fixed point with 8 fractional bits, so that the cell arithmetic stays exact integer:
 *        p_a is first clamped in floating point to [-1/2, S_a - 1/2] (NaN -> the low edge, -inf / +inf -> the nearer edge);
 *        t_a = rint(256 p_a) + 128 (round half to even; 256 p_a is exact), clamped to [0, 256 S_a - 1];
 *        per level q = t_a R_l as an exact integer (< 2^38), v_a = q div (256 S_max), w_a = fp32(q mod 256 S_max) / fp32(256 S_max).
 *      Entry index, corner weights, blend and column layout are nic_hash_encode's, unchanged.  Consequences:
 *      - at a sample centre t = 128 (2 i + 1): q is 128 times the lattice route's q and the divisor 128 times its 2 S_max, so v is identical
 *        and w is the same fp32 quotient (scaling both operands by a power of two is exact): the row equals nic_hash_encode's bit for bit
 *        (and nic_hash_encode_noisy's / _u8's / _bits' for the other sources, the noise keyed by sample_base + n and the column);
 *      - the upper clamp keeps v_a <= R_l - 1, corner v + 1 never exceeds R_l: a dense level of the compact uint8 or packed table is never
 *        read past its E_l entries, and no input - out of range, NaN, infinite - can address outside a level; a point outside the field gives
 *        exactly the row of the clamped point.
 *      Host checks on top of nic_hash_encode's, all before any GPU work, codes in the order of the crop siblings (descriptor, null pointers,
 *      arguments): 256 S_max < 2^30 (else NIC_E_ARG; every field the descriptor accepts at 4K or 256^3 passes); the source: kind one of
 *      NIC_HASH_SRC_*, num_bits 0 for F32 and 1 .. 8 for U8 / BITS, a BITS table 4-byte aligned (else NIC_E_ARG); `quant` (null, or the
 *      noise of nic_hash_encode_noisy) only with an F32 source (else NIC_E_ARG); n_points < 0 is NIC_E_ARG, n_points == 0 is NIC_OK with
 *      no launch.  nic_hash_encode_points_backward is the straight-through scatter of nic_hash_encode_backward (ADDS into table_grad, fp32
 *      atomics, order not fixed).  nic_hash_fused_forward_points is nic_hash_fused_forward / _u8 / _bits at points ([n_points, 3]; the set
 *      nic_hash_fused_supported answers for).  Training at points in cell order and in one fused kernel: the next section. */
#define NIC_HASH_SRC_F32 0   /* fp32 [levels, T, features] table */
#define NIC_HASH_SRC_U8 1    /* compact uint8 table (nic_hash_pack_u8) */
#define NIC_HASH_SRC_BITS 2  /* bit-packed table (nic_hash_pack_bits) */
typedef struct nic_hash_source {
    int32_t kind;            /* NIC_HASH_SRC_F32 / _U8 / _BITS */
    int32_t num_bits;        /* 1 .. 8 for U8 / BITS, 0 for F32 */
    const void *data;
} nic_hash_source;
int nic_hash_encode_points(const nic_hash_desc *desc, const nic_hash_source *src, const nic_hash_quant *quant, const float *points,
                           int64_t n_points, float *out, void *stream);
int nic_hash_encode_points_backward(const nic_hash_desc *desc, const float *points, int64_t n_points, const float *dx, float *table_grad,
                                    void *stream);
int nic_hash_fused_forward_points(const nic_hash_desc *desc, const nic_hash_source *src, const float *points, int64_t n_points,
                                  const nic_mlp *mlp, float *y, void *stream);

/* ---- cell-ordered and fused training at points (hashgrid.py, HashGridField.train_points(order=, fused=) / fit_points).
 *      nic_hash_point_keys: keys[n] = the Morton key of point n, a pure function of the clamped fixed-point position defined above:
 *        t_a as above (p_a clamped in floating point - NaN to the low edge, -inf / +inf to the nearer one - then rint(256 p_a) + 128 clamped to
 *        [0, 256 S_a - 1]); b = the bit length of 256 S_max - 1 (<= 30), k = 31 for dim 2 and 21 for dim 3, s = max(0, b - k), u_a = t_a >> s;
 *        bit j of u_a goes to bit j dim + a of the key.  0 <= key < 2^63.  Z-order of position is hierarchical: neighbours in key order share
 *        their cell at the coarse levels and mostly at the fine ones, so a launch that walks the points in key order (a stable sort of the keys,
 *        the caller's) sums neighbouring lanes of one cell before the atomics.  One lane per point; keys = [n_points] int64 (device).
 *      nic_hash_encode_points_backward_ordered: nic_hash_encode_points_backward with lane n of the launch on point order[n] - it reads
 *        points[order[n]] and row order[n] of dx.  order = [n_points] int32 (device; the host never reads it); every index is clamped to
 *        [0, n_points - 1] by the kernel, so a buffer that is no permutation gives the sum over the rows it names and never an access out of
 *        range.  order == NULL is nic_hash_encode_points_backward itself; n_points >= 2^31 with an order is NIC_E_ARG.
 *      nic_hash_fused_forward_backward_points: nic_hash_fused_forward_backward with the samples taken from `points` through the cell arithmetic
 *        of nic_hash_encode_points - two launches (the fused kernel, then the fixed-order reduction of its per-workgroup records with `tail`
 *        riding on it), loss = mean((y - target)^2) loss_scale over the [n_points, 3] outputs, table_grad ADDED into (null: frozen table, no
 *        scatter), NIC_HASH_FUSED_ADD_GRADS / _ADD_LOSS, y null or [n_points, 3], nic_mark_kernel_end honoured.  With `order`, wave w handles
 *        points order[64 w .. 64 w + 63]: target is read and y written at row order[n], the noise keyed by sample_base + order[n] and the
 *        column - an ordered call computes the unordered call's function up to the order of the sums, with noise too.  Indices are clamped as
 *        above.  Supported: what nic_hash_fused_supported answers for, plus num_crops == 1 and 256 S_max < 2^30 of the point entries.
 *      Host checks, all before any GPU work, in the order of the siblings: descriptor (fused set first for the fused entry), null pointers,
 *      flags / quant, n_points < 0 or n_points >= 2^31 with an order (NIC_E_ARG), workspace < nic_hash_fused_points_workspace_bytes
 *      (NIC_E_WORKSPACE; the query returns 0 for what the entry refuses), the tail (its decoder gradients must be this call's mlp_grads, else
 *      NIC_E_ARG).  n_points == 0 is NIC_OK with no launch and leaves *loss untouched. */
int nic_hash_point_keys(const nic_hash_desc *desc, const float *points, int64_t n_points, int64_t *keys, void *stream);
int nic_hash_encode_points_backward_ordered(const nic_hash_desc *desc, const float *points, int64_t n_points, const float *dx,
                                            const int32_t *order, float *table_grad, void *stream);
size_t nic_hash_fused_points_workspace_bytes(const nic_hash_desc *desc, const nic_mlp *mlp);   /* 0: unsupported */
int nic_hash_fused_forward_backward_points(const nic_hash_desc *desc, const nic_hash_quant *quant, const float *table, const float *points,
                                           int64_t n_points, const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                           float *table_grad, const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags, void *workspace,
                                           size_t workspace_bytes, const nic_step_tail *tail, void *stream);

/* ---- hash-grid codec: a bit depth PER LEVEL (hashgrid.py, HashGridField(num_bits=[b_0, ..]); csrc/hash_mixed.hip).
 *      level_bits->bits[l] = b_l in 1 .. 8 for each of desc->levels levels (entries past desc->levels are ignored); everything is the codec
 *      above applied per level with b = b_l:
 *      - clamp range of level l: [-(2^b_l - 1) / 2^(b_l + 1), 1/2] (nic_hash_clamp_levels, in place on the fp32 [L, T, F] table, NaN kept);
 *      - noise: columns l F + f take nic_hash_encode_noisy's value with scale 2^-b_l.  Block numbering, the Threefry keys, the sample_base +
 *        row keying and the value's expression are unchanged, only the power-of-two scale is the level's: equal depths give
 *        nic_hash_encode_noisy's row bit for bit.  quant->num_bits is ignored by these entry points;
 *      - stored format nicv2-hashgrid-bits/2 = format /1 with b replaced by b_l inside level l: value f of entry e of level l occupies bits
 *        [(e F + f) b_l, (e F + f + 1) b_l) of that level's little-endian stream, each level is padded to whole dwords and starts at byte
 *        4 sum_{k<l} ceil(E_k F b_k / 32), 8 zero bytes follow the last level; nic_hash_packed_bytes_levels = 4 sum_l ceil(E_l F b_l / 32) + 8
 *        (host arithmetic; or a negative NIC_E_* code).  The stored value and its dequantisation are nic_hash_pack_u8's / nic_hash_encode_u8's
 *        expressions with b_l: level l of a mixed table holds exactly the bytes level l of a /1 table of depth b_l holds and decodes to exactly
 *        its columns.  nic_hash_pack_bits_levels writes the whole buffer (padding and tail as zeros, one dword per thread, no atomics).  There
 *        is no uint8 form of a mixed table.
 *      Positions: exactly one of `origins` / `points` is non-null (else NIC_E_ARG).  origins = the crop lattice of nic_hash_encode (rows,
 *      noise keys and outputs in its sample order; n_points ignored); lattice sample i is taken as the point t = 256 i + 128, which gives the
 *      crop route's row bit for bit (previous section), so the lattice route needs 256 S_max < 2^30 too.  points = as in
 *      nic_hash_encode_points (desc->extent the field size, num_crops 1).
 *      Source (src): NIC_HASH_SRC_F32, or NIC_HASH_SRC_BITS = a format /2 table, 4-byte aligned; NIC_HASH_SRC_U8 is NIC_E_ARG and
 *      src->num_bits must be 0.  `quant` (null or kernel noise, then per-level noise) only with an F32 source.
 *      nic_hash_encode_levels: the [N, L F] row.  nic_hash_fused_forward_levels: gather + decoder in one launch ([N, 3]; the set
 *      nic_hash_fused_supported answers for).  nic_hash_fused_forward_backward_levels: nic_hash_fused_forward_backward_points' contract with
 *      per-level noise and either position source - two launches, the second the fixed-order reduction with `tail` riding on it; `order` only
 *      with `points` (else NIC_E_ARG); workspace >= nic_hash_fused_points_workspace_bytes (the size does not depend on the crops).
 *      The straight-through scatter does not depend on the depth: nic_hash_encode_backward / nic_hash_encode_points_backward(_ordered) serve
 *      the layer-wise backward as they are.  Every argument error is returned on the host before any GPU work, codes and order as in the
 *      _points siblings (descriptor, the position pair, null pointers, depths outside 1 .. 8, source, quant, n_points, workspace, tail). */
typedef struct nic_hash_level_bits {
    int32_t bits[NIC_HASH_MAX_LEVELS];
} nic_hash_level_bits;
int64_t nic_hash_packed_bytes_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits);
int nic_hash_pack_bits_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits, const float *table, uint8_t *packed, void *stream);
int nic_hash_clamp_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits, float *table, void *stream);
int nic_hash_encode_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits, const nic_hash_source *src,
                           const nic_hash_quant *quant, const int32_t *origins, const float *points, int64_t n_points, float *out, void *stream);
int nic_hash_fused_forward_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits, const nic_hash_source *src,
                                  const int32_t *origins, const float *points, int64_t n_points, const nic_mlp *mlp, float *y, void *stream);
int nic_hash_fused_forward_backward_levels(const nic_hash_desc *desc, const nic_hash_level_bits *level_bits, const nic_hash_quant *quant,
                                           const float *table, const int32_t *origins, const float *points, int64_t n_points,
                                           const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale, float *table_grad,
                                           const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags, void *workspace,
                                           size_t workspace_bytes, const nic_step_tail *tail, void *stream);

/* ---- the hash-grid field at points with a level of detail PER POINT (hashgrid.py, HashGridField.query / train_points(lod=), decode_mip,
 *      fit_mips; csrc/hash_points.hip, csrc/hash_points_train.hip).  What a texture sampler has: lambda fades the levels finer than a query's footprint out,
 *      before the decoder.
 *      - lambda of point n = (lod ? lod[n] : 0) + lod_uniform in fp32; NaN becomes 0; the sum is then clamped to [0, 32].  lod = [n_points]
 *        fp32 (device; the host never reads it) or NULL; with an `order` it is read at order[n] like the point.
 *      - weight of level l: a_l = min(max((fade[l] - lambda) + 1.0f, 0), 1) in fp32, in exactly this order (one subtract, one add: nothing
 *        contracts).  Level l is fully on up to lambda = fade[l] and off from fade[l] + 1.  fade[l] is the caller's; hashgrid.hash_lod_fade gives
 *        max(0, log2(S_max / R_l)) (float64, rounded once), the level's cell size in octaves of samples: every weight is exactly 1 at lambda = 0.
 *      - column l F + f of the row is fl(a_l r), r the value nic_hash_encode_points produces (the blend, plus the noise of `quant`): at
 *        a_l = 1 the row is that entry's bit for bit.  A level of weight 0 contributes exactly 0 - no noise either - and its table is not read;
 *        a level no lane of a wave weighs above 0 costs that wave no gather at all.
 *      - backward: straight-through, dx of level l multiplied by a_l (fl(a_l dx) goes where nic_hash_encode_points_backward(_ordered) sends dx);
 *        a point with a_l = 0 issues no atomic for level l, a level nobody weighs is not touched.
 *      Everything else - fixed-point positions, cells, entry index, the three sources, the noise keys (sample_base + n, or + order[n] in the
 *      fused step), the clamped `order` - is that of the entries without _lod, argument for argument:
 *      nic_hash_encode_points_lod = nic_hash_encode_points; nic_hash_encode_points_backward_lod = nic_hash_encode_points_backward_ordered
 *      (order may be NULL); nic_hash_fused_forward_points_lod = nic_hash_fused_forward_points; nic_hash_fused_forward_backward_points_lod =
 *      nic_hash_fused_forward_backward_points: two launches, records, tail, flags and workspace exactly as there - the workspace query is
 *      nic_hash_fused_points_workspace_bytes.  A bit depth per level (nic_hash_level_bits) is not served by these entries.
 *      Host checks, all before any GPU work, in the siblings' order and with their codes (descriptor, null pointers, arguments); on top of
 *      them lodp == NULL is NIC_E_NULL (with the other pointers), and right after the pointers a fade[l] (l < levels) that is not finite or is
 *      negative, a lod_uniform that is not finite, or reserved != 0 is NIC_E_ARG.  fade entries past desc->levels are ignored. */
typedef struct nic_hash_lod {
    float fade[NIC_HASH_MAX_LEVELS];   /* finite, >= 0 */
    float lod_uniform;                 /* finite; added to every point's lod */
    int32_t reserved;                  /* 0 */
} nic_hash_lod;
int nic_hash_encode_points_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const nic_hash_quant *quant,
                               const float *points, const float *lod, int64_t n_points, float *out, void *stream);
int nic_hash_encode_points_backward_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const float *points, const float *lod,
                                        int64_t n_points, const float *dx, const int32_t *order, float *table_grad, void *stream);
int nic_hash_fused_forward_points_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const float *points,
                                      const float *lod, int64_t n_points, const nic_mlp *mlp, float *y, void *stream);
int nic_hash_fused_forward_backward_points_lod(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_quant *quant,
                                               const float *table, const float *points, const float *lod, int64_t n_points,
                                               const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                               float *table_grad, const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags,
                                               void *workspace, size_t workspace_bytes, const nic_step_tail *tail, void *stream);

/* ---- the forward-only fused routes with the decoder on the 16-bit matrix pipe (hashgrid.py, HashGridField.decode / query / resample
 *      (precision=); csrc/hashgrid_fused16.hip).  nic_hash_fused_forward / _u8 / _bits (origins) and
 *      nic_hash_fused_forward_points (points) with the products of the three Linear layers taken in 16-bit operands; y is [N, 3] in the
 *      sample order of those entries.  One launch, no atomics: the same call gives the same bits.
 *      - the row x [L F] is the existing route's, bit for bit: nic_hash_encode / _u8 / _bits on the lattice, nic_hash_encode_points at points.
 *      - per layer, W the fp32 nn.Linear weight and a the fp32 input (the row, then the fp32 GELU outputs), hi = bf16_rne(v),
 *        lo = bf16_rne(v - hi) for both operands:
 *          NIC_HASH_PREC_SPLIT  z = sum_k (a_lo W_hi + a_hi W_lo + a_hi W_hi)   products exact, fp32 accumulation, no lo x lo term
 *          NIC_HASH_PREC_BF16   z = sum_k a_hi W_hi                             products exact, fp32 accumulation
 *        the bias is added in fp32; GELU and the output sigmoid are the fp32 functions of the fp32 route.  Columns past L F and output rows
 *        3 .. 31 of the matrix tiles are exact zero padding.  The modes differ from the fp32 route in the products alone.
 *      Positions: exactly one of `origins` / `points` is non-null (else NIC_E_ARG), as in nic_hash_fused_forward_levels: a lattice sample i
 *      is the point t = 256 i + 128, so the lattice route needs 256 S_max < 2^30 too; n_points is ignored with `origins`.
 *      Source (src): NIC_HASH_SRC_F32, _U8 or _BITS with the rules of nic_hash_encode_points (num_bits 0 for F32 and 1 .. 8 for U8 / BITS, a
 *      BITS table 4-byte aligned).  Supported: what nic_hash_fused_supported answers for.  No level of detail, no bit depth per level.
 *      Every argument error is returned on the host before any GPU work, in the order of nic_hash_fused_forward_levels: null desc / mlp,
 *      nic_hash_fused_supported, the position pair, the descriptor of that position source, null pointers, the source, `precision` not
 *      NIC_HASH_PREC_SPLIT or NIC_HASH_PREC_BF16 (NIC_E_ARG), n_points < 0 (NIC_E_ARG); n_points == 0 at points is NIC_OK without a launch. */
#define NIC_HASH_PREC_SPLIT 1
#define NIC_HASH_PREC_BF16 2
int nic_hash_fused_forward_p16(const nic_hash_desc *desc, const nic_hash_source *src, const int32_t *origins, const float *points,
                               int64_t n_points, const nic_mlp *mlp, int precision, float *y, void *stream);

/* ---- gradients with respect to the POINT COORDINATES (hashgrid.py, HashGridField.point_gradient / jacobian / query_differentiable;
 *      csrc/hashgrid_pointgrad.hip).  The spatial derivative of what the field represents.
 *      Notation is that of nic_hash_encode_points: p_a in sample units, clamped to [-1/2, S_a - 1/2]; t_a = rint(256 p_a) + 128, clamped; per
 *      level q = t_a R_l, v_a and w_a from the cell arithmetic there.  Column l F + f of the row is a_l sum_c prod_b cw_b(c) value[l, idx(v + c), f]
 *      with cw_b(c) = c_b ? w_b : 1 - w_b and a_l = 1 without a level of detail.  One sample is 1/256 of 256 p_a and one cell of level l is
 *      256 S_max / R_l of those units, so d w_a / d p_a = R_l / S_max, and
 *
 *        d row[l F + f] / d p_a  =  a_l (R_l / S_max) sum_c (c_a ? +1 : -1) prod_{b != a} cw_b(c) value[l, idx(v + c), f]
 *        dpoints[n, a]           =  sum_l sum_f dx[n, l F + f] d row[l F + f] / d p_a
 *
 *      - the interpolant, at the rounded position: the derivative of the multilinear interpolant at the position the forward route uses (the
 *        1/256 rounding and the integer clamp of t are passed straight through).  It is piecewise constant along its own axis inside a cell
 *        and discontinuous across cell faces; there is no smoothstep variant.
 *      - clamped axes: axis a of a point whose floating-point clamp changed p_a (p_a < -1/2, p_a > S_a - 1/2, NaN, -inf / +inf) gives exactly
 *        0.0f on that axis; its other axes are those of the clamped point, bit for bit.  p_a = S_a - 1/2 itself is not clamped and takes the
 *        last cell's derivative.
 *      - values: what the forward route blends - the fp32 entry, or the dequantised uint8 / bit-packed entry (both window forms of the packed one).
 *      - noise is additive on the row and does not enter.
 *      - level of detail: lodp == NULL is none (then lod must be NULL too, else NIC_E_ARG); else a_l is nic_hash_encode_points_lod's and depends
 *        on lambda only: a level of weight 0 is not gathered and adds nothing, a level no lane of a wave weighs is skipped by the wave.  There is
 *        no gradient with respect to lambda from these two entries: the _grad_lod entries of nicv2_hip_ext.h give it next to dpoints.
 *      - outputs are WRITTEN, not added; row n belongs to point n; there are no atomics: the same call gives the same bits.
 *      nic_hash_encode_points_grad: dx = [n_points, L F] (d loss / d row), dpoints = [n_points, dim]; one lane per point; the three sources,
 *        dim 2 / 3, features 1 / 2 / 4 / 8.
 *      nic_hash_fused_points_grad: one launch for the set nic_hash_fused_supported answers for (plus num_crops == 1 and 256 S_max < 2^30): the
 *        row of nic_hash_encode_points(_lod) stays on the chip, y = ColorDecoder(row) as nic_hash_fused_forward_points(_lod) (y null or
 *        [n_points, 3]), then the decoder's backward to its input with the products of nic_hash_fused_forward_backward_points in their order -
 *        dZ3 = dy y (1 - y), dA2 = W3^T dZ3, dZ2 = dA2 gelu', dA1 = W2^T dZ2, dZ1 = dA1 gelu', dx = W1^T dZ1 - and dpoints from that dx.
 *        Exactly one of dy / target ([n_points, 3]) is non-null: with target, dy = 2 (y - target) loss_scale / (3 n_points), the gradient of
 *        mean((y - target)^2) loss_scale; loss_scale is ignored with dy.  The loss is not an output (the caller has y).  The decoder and the
 *        table are constants: no parameter gradient, no workspace, no reduction launch.
 *      Host checks, all before any GPU work, in the siblings' order and with their codes: descriptor (null desc / mlp, then the fused set, for
 *      the fused entry), null pointers (src, src->data, points, dx / the decoder's layers, dpoints), the source (nic_hash_encode_points' rules),
 *      the nic_hash_lod (nic_hash_encode_points_lod's rules), both or neither of dy / target (NIC_E_ARG), n_points < 0 (NIC_E_ARG);
 *      n_points == 0 is NIC_OK with no launch. */
int nic_hash_encode_points_grad(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const float *points,
                                const float *lod, int64_t n_points, const float *dx, float *dpoints, void *stream);
int nic_hash_fused_points_grad(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_source *src, const float *points,
                               const float *lod, int64_t n_points, const nic_mlp *mlp, const float *dy, const float *target, float loss_scale,
                               float *y, float *dpoints, void *stream);

/* ---- the field AND the point positions in one training step (hashgrid.py, HashGridField.train_points(dpoints=) /
 *      train_points_differentiable; csrc/hashgrid_points_joint.hip).
 *      nic_hash_fused_forward_backward_points_grad: with lodp == NULL it is nic_hash_fused_forward_backward_points, otherwise
 *      nic_hash_fused_forward_backward_points_lod, argument for argument - two launches, the per-workgroup records, the fixed-order reduction
 *      with `tail` riding on it, NIC_HASH_FUSED_ADD_GRADS / _ADD_LOSS, the workspace (the query is nic_hash_fused_points_workspace_bytes), the
 *      noise keys (sample_base + order[n] and the column), the clamped `order`, nic_mark_kernel_end, the fp32 table as the only source.  loss,
 *      y and the decoder gradients are those entries' bit for bit; table_grad is theirs up to the order of the atomics.
 *      On top of that row n of dpoints [n_points, dim] is written once, by the lane that handles point n (with an `order` that is row order[pos],
 *      not pos): d loss / d points[n] of the loss this call returns, loss_scale mean((y - target)^2) over the call's points -
 *      nic_hash_fused_points_grad's value with `target`, bit for bit.  The derivative is taken at the parameters the forward used (before the
 *      tail's step), with the codec noise and the level weights as constants, as the derivative of the multilinear interpolant at the rounded
 *      position (previous section), in sample units, exactly 0.0f on an axis whose floating-point clamp moved the point.  dpoints is
 *      OVERWRITTEN, never added to, whatever NIC_HASH_FUSED_ADD_GRADS says; no atomic touches it: the same call gives the same bits.
 *      table_grad == NULL is a frozen table: no scatter; dpoints and the decoder records are still produced.
 *      Host checks, all before any GPU work, with the siblings' codes, in this order: null desc / mlp, the fused set
 *      (nic_hash_fused_supported), the conditions of the point entries (num_crops == 1, 256 S_max < 2^30), null pointers (table, points, the
 *      decoder's layers, target, mlp_grads, loss, dpoints, workspace: NIC_E_NULL; lodp, lod, order, table_grad, y and tail may be null), flags
 *      outside the two above (NIC_E_ARG), the nic_hash_lod when given (nic_hash_encode_points_lod's rules), lodp == NULL with lod != NULL
 *      (NIC_E_ARG, nic_hash_fused_points_grad's rule), quant, n_points < 0 or n_points >= 2^31 with an order (NIC_E_ARG), the workspace
 *      (NIC_E_WORKSPACE), the tail.  n_points == 0 is NIC_OK with nothing written. */
int nic_hash_fused_forward_backward_points_grad(const nic_hash_desc *desc, const nic_hash_lod *lodp, const nic_hash_quant *quant,
                                                const float *table, const float *points, const float *lod, int64_t n_points,
                                                const int32_t *order, const nic_mlp *mlp, const float *target, float loss_scale,
                                                float *table_grad, const nic_mlp_grads *mlp_grads, float *loss, float *y, float *dpoints,
                                                int flags, void *workspace, size_t workspace_bytes, const nic_step_tail *tail, void *stream);

/* ---- B hash-grid fields of one geometry per launch (hashgrid.py, HashGridFieldBatch; csrc/hashgrid_batch.hip).
 *      All n_fields fields share `desc`: dim, levels, features, log2_table, resolutions, the crop extent and num_crops.  Storage is stacked and
 *      contiguous, and the field strides follow from desc - the arguments are the BASES: tables and table_grads [B, L, T, F] fp32; mlp / mlp_grads
 *      the bases of W1 [B, 64, L F], b1 [B, 64], W2 [B, 64, 64], b2 [B, 64], W3 [B, 3, 64], b3 [B, 3]; origins [B, num_crops, dim] int32 on the
 *      device (every field has its own crops); target and y [B, N, 3], N = num_crops x the extents; loss [B].
 *      nic_hash_batch_forward is nic_hash_fused_forward per field in ONE launch, nic_hash_batch_forward_backward is
 *      nic_hash_fused_forward_backward per field in TWO launches (the training kernel and the fixed-order reduction of its records) whatever
 *      n_fields is: loss[b] = loss_scale mean((y_b - target_b)^2) over field b's N samples, table_grads (null: frozen tables, no scatter) is
 *      ADDED to with fp32 atomics, the decoder gradients are overwritten (NIC_HASH_FUSED_ADD_GRADS: added to), likewise loss
 *      (NIC_HASH_FUSED_ADD_LOSS); y null or [B, N, 3]; nic_mark_kernel_end honoured.  The noise of `quant` is keyed by sample_base + the row
 *      INSIDE the field and the column: field b sees exactly the noise of a single-field call with the same quant.  There is no optimiser
 *      tail: one nic_adam_multi over the stacked tensors steps every field.  Against the single-field entries y, loss and the gradients agree
 *      to the summation order (the records of a field are split over other workgroups).
 *      A workgroup belongs to one field: field b has groups_per_field = G workgroups, the launch n_fields x G.  G = 0 is automatic: the
 *      workgroup cap of a persistent launch (one per CU, a multiple of 8) / n_fields, rounded up to a multiple of 8, at least 8, at most the
 *      grid nic_hash_fused_forward would use for one field.  A positive G must be a multiple of 8 and at most that grid.  n_fields x G may exceed
 *      the CU count (nothing synchronises across workgroups).  workspace >= nic_hash_batch_workspace_bytes (n_fields x G records; 0: refused).
 *      Host checks, all before any GPU work, in nic_hash_fused_forward_backward's order: null desc / mlp (NIC_E_NULL), the fused set
 *      (nic_hash_fused_supported's code; then 256 S_max < 2^30, NIC_E_ARG: the lattice is read through the fixed-point cell), n_fields in
 *      1 .. 65535 (NIC_E_ARG), groups_per_field (NIC_E_ARG), null pointers (NIC_E_NULL; table_grads and y may be null), flags (NIC_E_ARG), quant
 *      (nic_hash_fused_forward_backward's rules), the workspace (NIC_E_WORKSPACE). */
size_t nic_hash_batch_workspace_bytes(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_mlp *mlp);   /* 0: refused */
int nic_hash_batch_forward(const nic_hash_desc *desc, int n_fields, int groups_per_field, const float *tables, const int32_t *origins,
                           const nic_mlp *mlp, float *y, void *stream);
int nic_hash_batch_forward_backward(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_quant *quant,
                                    const float *tables, const int32_t *origins, const nic_mlp *mlp, const float *target, float loss_scale,
                                    float *table_grads, const nic_mlp_grads *mlp_grads, float *loss, float *y, int flags, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* ---- B STORED fields per launch, on the lattice or at points (hashgrid.py, HashGridFieldBatch.load_compressed / decode / query / resample,
 *      hash_batch_forward_source; csrc/hashgrid_batch.hip).  Forward only: one launch, no atomics, no records - the same call
 *      gives the same bits.  nic_hash_batch_forward_source is nic_hash_fused_forward / _u8 / _bits (origins) or nic_hash_fused_forward_points
 *      (points) per field in ONE launch; workgroups belong to fields as above, the decoder is the stacked one of nic_hash_batch_forward.
 *      Source: src->kind NIC_HASH_SRC_F32, _U8 or _BITS with the rules of nic_hash_encode_points (num_bits 0 for F32 and 1 .. 8 for U8 / BITS),
 *      src->data the BASE of n_fields tables stacked without gaps: field b's table starts b x stride bytes after it, stride = levels x T x
 *      features x 4 (F32), nic_hash_stored_bytes(desc) (U8) or nic_hash_packed_bytes(desc, num_bits) (BITS).  The BITS stride is 4 x sum + 8, a
 *      multiple of 4: a 4-byte-aligned base (else NIC_E_ARG) aligns every field, and each field keeps its own 8 zero bytes.
 *      Positions: exactly one of `origins` / `points` is non-null (else NIC_E_ARG), as in nic_hash_fused_forward_p16.  origins = [B, num_crops,
 *      dim] int32 on the device (every field its own crops), y = [B, N, 3] in nic_hash_batch_forward's order; n_points is ignored.  points =
 *      [B, n_points, dim] fp32 on the device in sample units with the clamping of nic_hash_encode_points (every field its own points), then
 *      desc->extent is the FIELD size, desc->num_crops is 1 and 256 S_max < 2^30, and y = [B, n_points, 3].  One wave handles 64 consecutive
 *      points of one field; a lane past the end decodes the field's last point and stores nothing.
 *      groups_per_field = G as above, on the wave items of ONE field: its patches with origins, ceil(n_points / 64) with points (0: automatic;
 *      a positive G must be a multiple of 8 and at most the grid a single-field launch over those items would use).
 *      Host checks, all before any GPU work, in this order: null desc / mlp (NIC_E_NULL); the fused set (nic_hash_fused_supported's code); both
 *      or neither of origins / points (NIC_E_ARG); the descriptor of that position source (points: num_crops == 1, NIC_E_SHAPE, and 256 S_max <
 *      2^30, NIC_E_ARG; origins: 256 S_max < 2^30, NIC_E_ARG); n_fields in 1 .. 65535 (NIC_E_ARG); groups_per_field (NIC_E_ARG; for this check
 *      alone n_points <= 0 counts as one wave item); null src, src->data, decoder layer or y (NIC_E_NULL); the source (NIC_E_ARG: kind,
 *      num_bits, alignment, in nic_hash_encode_points' order); n_points < 0 with points (NIC_E_ARG); n_points == 0 with points is NIC_OK
 *      without a launch. */
int nic_hash_batch_forward_source(const nic_hash_desc *desc, int n_fields, int groups_per_field, const nic_hash_source *src,
                                  const int32_t *origins, const float *points, int64_t n_points, const nic_mlp *mlp, float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NICV2_HIP_H */
