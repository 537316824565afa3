/*
 * dasac_hip.h -- C-ABI of libdasac_hip.so: the MI355X (gfx950) kernels under the da-sac
 * per-step hot path.
 *
 * The reference (visinf/da-sac) has no FFI of its own: every kernel it runs is an implicit
 * ATen/cuDNN call made from models/{sac,deeplabv2,fcn,basenet}.py.  This header is the new
 * seam directly under those modules; each entry point names the reference
 * lines whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; NCHW contiguous fp32 activations / weights, int64 labels
 *     (255 = ignore), bool masks as uint8;  no torch types anywhere in a signature;
 *   - an OPERAND (activation, weight, gradient, label, image, bit mask, packed GEMM operand) needs the alignment of its
 *     element and no more, and the result does not depend on where it lies; only what the text of an entry names needs more:
 *     control blocks and workspaces, the dasac_conv_gemm_batched strides, and the DESCRIPTOR tables the kernels read as 16- or
 *     8-byte records (gather tables; job, pair and row tables; chunk lists).  A descriptor off its alignment is DASAC_EINVAL
 *     before any launch;
 *   - `stream` is a hipStream_t (NULL = the legacy default stream);
 *   - return 0 on success, a negative DASAC_E* code otherwise; never throws, never allocates
 *     device memory, never synchronises the stream.  Scratch comes from the caller:
 *     `dasac_*_workspace(...)` returns the bytes a call needs (16-byte aligned pointer);
 *   - re-entrant per stream; dasac_last_error() is thread-local.
 */
#ifndef DASAC_HIP_H
#define DASAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DASAC_OK 0
#define DASAC_EINVAL (-1)   /* bad argument (null pointer, shape, unsupported geometry) */
#define DASAC_EWORKSPACE (-2) /* workspace too small */
#define DASAC_ELAUNCH (-3)  /* HIP launch / runtime error, see dasac_last_error() */

typedef void* dasac_stream_t; /* hipStream_t */

int dasac_version(void);                 /* ABI version, currently 1 */
const char* dasac_last_error(void);      /* thread-local message of the last failure */
int dasac_device_info(int* cu_count, int* wave_size, char* arch, size_t arch_len);
/* Compute units this process leaves to kernels that run beside its own -- RCCL's all-reduce kernels when the gradient
 * reduction is overlapped with the backward pass (train.py:104 DistributedDataParallel; here dasac_hip.parallel).  The
 * persistent stream-K grid (3 workers per CU, equal matrix work per worker) and the grid cap of the streaming kernels are
 * sized to 256 - n CUs, so that a collective's workgroups do not land on CUs whose workers then finish last.  n is rounded
 * up to a multiple of 8 and capped at 128; 0 (the default, or DASAC_SK_RESERVE_CUS in the environment) = the whole chip.
 * dasac_set_reserved_cus returns the previous value.  Results do not depend on n beyond the summation order of stream-K tiles. */
int dasac_reserved_cus(void);
int dasac_set_reserved_cus(int n);

/* ------------------------------------------------------------------------------------------
 * Pseudo-label extraction -- models/sac.py:154-187 (`SAC._pseudo_labels_probs`).
 *   (m,k) = max/argmax_c probs (ties -> lowest c);  peak[b,c] = max{m : k == c};
 *   thr[b,c] = max(peak*upper*disc[c], lower)  (fp32, that op order; disc may be NULL);
 *   labels = k if m > thr[b,k] else 255;  labels = 255 where ignore != 0.
 * probs [B,C,HW] f32, ignore [B,HW] u8 (may be NULL), labels [B,HW] i64, max_conf [B,HW] f32,
 * max_idx [B,HW] i64 (may be NULL: the reference never reads it, sac.py:357).  Requires
 * lower > 0 and C <= 64.  Integer outputs are bit-exact w.r.t. the CPU reference.
 */
size_t dasac_pseudo_labels_workspace(int B, int C, int64_t HW);
int dasac_pseudo_labels(const float* probs, const uint8_t* ignore, const float* disc,
                        float upper, float lower, int B, int C, int64_t HW,
                        int64_t* labels, float* max_conf, int64_t* max_idx,
                        void* workspace, size_t ws_bytes, dasac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Convolutions as implicit GEMM on fp32 MFMA -- every nn.Conv2d of models/deeplabv2.py
 * (:59,65-66,70,107,122,147-148,262-263) and models/fcn.py (:49,53,57,78,88), with the
 * BN(eval)/bias/residual/ReLU chain of Bottleneck.forward (deeplabv2.py:79-99) in the epilogue.
 *
 * A convolution is described by "tap branches" (kh,kw,dilation,padding): one branch for a plain
 * conv, four for the ASPP sum of deeplabv2.py:112-116 evaluated as a single contraction.
 *   K = (sum of kh*kw) * C;  `order` 0: k = tap*C + c (tap-major, required by the weight gradient);
 *   `order` 1: k = ((c/16)*taps + tap)*16 + c%16 (chunk-major, C % 16 == 0: the taps of a 16-channel
 *   chunk are contracted back to back so their shifted re-reads stay in L2) -- table and packed
 *   weights of one GEMM must use the same order.
 * dasac_conv_table   builds the gather table [Kpad][4] int32 for planes of plane_h x plane_w;
 *                    transposed=1 gives the data-gradient geometry (C = Cout, dh = pad - kh*dil).
 *                    The table is read one 16-byte row at a time: `table` must be 16-byte aligned here and in every entry
 *                    that takes it (dasac_conv_gemm, _stats, _x3, _batched, dasac_conv_wgrad, _x3).
 * dasac_conv_pack    lays W [Cout,Cin,kh,kw] out as the k-interleaved [Kpad/4][Mpad][4] GEMM operand
 *                    (transposed=1: rows (tap,co), columns ci), optionally scaled per co by
 *                    `scale` = folded BN gamma*invstd -- forward and data-gradient both contract
 *                    against scale*W, so the epilogue only adds the shift.
 *                    Call once per branch (tap0 = first tap of the branch, total_taps = all).
 * dasac_conv_gemm    out[n,m,oh*os,ow*os] = epi( sum_k packed[k][m] * x[n, c, oh*stride+dh, ow*stride+dw] )
 *                    epi: v + shift[m] (+res) (ReLU) (zeroed where mask <= 0 / where its mask bit is clear).
 *                    ReLU patterns may travel as ONE BIT per element instead of the fp32 activation:
 *                    `relu_bits_out` (with relu = 1) receives bit (pix & 31) of word [m][pix >> 5] = (out > 0), pix =
 *                    flattened (n, oh, ow) index, dasac_relu_bits_words(M, Nb*OH*OW) uint32 words; `mask_bits`
 *                    consumes such a pattern in the data-gradient GEMM whose output has the producer's shape
 *                    (1/32 of the mask bytes; exclusive with `mask`; both need ostride = 1 and
 *                    dasac_conv_gemm_bits_ok(M, Cx): the 128-row fp32 tile, Cx % 16 == 0).  The launch covers the
 *                    output pixels [pix_begin, pix_begin + pix_count) of the flattened (n, oh, ow) grid
 *                    (whole 128-pixel tiles; pix_count 0 = to the end); schedule 0 = pick, 1 = one block
 *                    per tile, 2 = persistent stream-K.  With a workspace of
 *                    dasac_conv_gemm_workspace() bytes (129 MB) schedule 0 may pick, for a long contraction whose
 *                    tile count leaves a ragged last round of resident workgroups: over the whole pixel range, ONE
 *                    launch of the leading whole rounds one block per tile + the remaining tiles cut into K-ranges
 *                    (split-K tail, dasac_conv_gemm_tail_split); with fewer tiles than resident workgroups, the
 *                    persistent stream-K schedule (equal matrix work per CU).  workspace NULL = one block per tile.
 *                    Every choice is a function of the shape and dasac_reserved_cus() alone: run-to-run identical bits.
 *                    The workspace must be ZERO-FILLED by the caller when it is allocated and belong to one
 *                    stream at a time: its hand-off flags are self-cleaning (every launch leaves them
 *                    zero), which saves a memset per launch.
 * dasac_conv_wgrad   partial weight gradients (split over pixels) into `workspace` of dasac_conv_wgrad_workspace bytes
 *                    (an upper bound over both k-tile widths, checked as it stands: anything less is DASAC_EWORKSPACE);
 * dasac_conv_wgrad_finish  sums the splits, writes dW[co,ci,kh,kw] = scale[co]*G and, when `dot`
 *                    is given (single-branch convolutions only), the frozen-BN gamma gradient term sum_k W*G as
 *                    dasac_conv_wgrad_dot_rows(Cin, taps) PARTIAL rows dot[row][co] (row = a block of 64 input
 *                    channels; every element is written, nothing to zero): dasac_bn_param_grads adds the rows in a
 *                    fixed order, no atomics, so two runs give the same bits; `sum_dz`
 *                    (optional) receives sum over batch and pixels of dz per channel (d beta / d bias),
 *                    accumulated for free by the wgrad kernel while it streams dz.
 */
int dasac_conv_mpad(int M);
int dasac_conv_kpad(int K);
int dasac_conv_table(const int32_t* kh, const int32_t* kw, const int32_t* dil, const int32_t* pad,
                     int n_branches, int C, int plane_h, int plane_w, int transposed, int order,
                     int32_t* table, dasac_stream_t stream);
int dasac_conv_pack(const float* w, const float* scale, int Cout, int Cin, int taps, int tap0,
                    int total_taps, int transposed, int order, float* packed, dasac_stream_t stream);
size_t dasac_relu_bits_words(int M, int64_t Npix);
int dasac_conv_gemm_bits_ok(int M, int Cx);   /* 1: dasac_conv_gemm takes mask_bits / relu_bits_out for this (M, gathered channels) */
int dasac_conv_gemm(const float* x, const float* packed, const int32_t* table, float* out,
                    int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                    int OutH, int OutW, int ostride,
                    const float* shift, const float* res, const float* mask,
                    const uint32_t* mask_bits, uint32_t* relu_bits_out,
                    int relu, int pix_begin, int pix_count, int schedule,
                    void* workspace, size_t ws_bytes, dasac_stream_t stream);
/* `batch` independent fp32 GEMMs of ONE geometry as one launch of the tile-per-block kernel (grid y = batch entry): entry b reads
 * x + b*x_stride and packed + b*packed_stride and writes out + b*out_stride (strides in ELEMENTS; the table is shared).  The other
 * arguments are dasac_conv_gemm's; there is no epilogue operand, pixel range, schedule or workspace: out = the plain contraction,
 * one workgroup per 128 x 128 tile, nothing handed between workgroups.  Inside an entry every address is the one
 * dasac_conv_gemm(schedule = 1) forms and the buffer windows are one entry's, so the result equals `batch` such calls bit for bit
 * and nothing outside an entry is read into a stored value or written.  Needs batch in 1..65535, Cx % 16 == 0, a padded M that is a
 * multiple of 128, every stride >= one entry's extent (Nb*Cx*H*W, dasac_conv_kpad(K)*dasac_conv_mpad(M), Nb*M*OutH*OutW) and a
 * multiple of 4 elements; batch = 1 may pass zero strides.  The 16 point GEMMs of a Winograd convolution are its user: 16 launches
 * that each fill a fraction of the chip's resident workgroup slots become one that fills whole rounds. */
int dasac_conv_gemm_batched(const float* x, const float* packed, const int32_t* table, float* out,
                            int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                            int OutH, int OutW, int ostride,
                            int batch, int64_t x_stride, int64_t packed_stride, int64_t out_stride,
                            dasac_stream_t stream);
/* Split-bf16 ("bf16x3") variant of the same contraction: every fp32 operand x is split into
 * head = bf16(x) and tail = bf16(x - head) and x*y is evaluated as xh*yh + xh*yl + xl*yh on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation (relative error of a product <= ~2^-15, typically
 * 2^-17; the dropped tail*tail term is below 2^-16).  The activations are split inside the kernel
 * (NCHW fp32 in HBM, nothing else changes), the weights once by dasac_conv_pack_x3 from the output of
 * dasac_conv_pack (same byte size).  Same table, epilogue, workspace and schedule as dasac_conv_gemm;
 * M must exceed 32.  Opt-in: the host picks it per call (DASAC_PRECISION=bf16x3 in the Python layer).
 * dasac_conv_pack_x3 reads `packed` and writes `packed_x3` (which may be `packed` itself) through 4-byte-aligned vectors:
 * both need element alignment only. */
int dasac_conv_pack_x3(const float* packed, int M, int K, void* packed_x3, dasac_stream_t stream);
int dasac_conv_gemm_x3(const float* x, const void* packed_x3, const int32_t* table, float* out,
                       int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                       int OutH, int OutW, int ostride,
                       const float* shift, const float* res, const float* mask,
                       const uint32_t* mask_bits, uint32_t* relu_bits_out,
                       int relu, int pix_begin, int pix_count, int schedule,
                       void* workspace, size_t ws_bytes, dasac_stream_t stream);
/* dasac_conv_gemm (fp32, no residual / mask / bit masks) whose epilogue ALSO leaves the per-channel statistics a
 * batch-statistics BatchNorm behind the convolution needs (nn.SyncBatchNorm in train mode: deeplabv2.py:15 with
 * models/__init__.py:29 BASELINE, train.py:281-289): stats [dasac_conv_gemm_stats_tiles(Nb, OH, OW)][2][dasac_conv_mpad(M)]
 * floats = per 128-pixel tile the sum and the sum of squares of every output row as stored (shift / bias included).  Every
 * slot is written by exactly one workgroup (also under the stream-K schedule); dasac_bn_train_finalize_tiles /
 * dasac_bn_tile_stats_reduce add the tiles in a fixed order -- no atomics, run-to-run identical.  Removes the stand-alone
 * statistics pass over the activation (one full read per BN layer).  Needs dasac_conv_gemm_stats_ok(M, Cx) (the 128-row
 * tile, Cx % 16 == 0) and ostride = 1. */
int dasac_conv_gemm_stats_ok(int M, int Cx);
int dasac_conv_gemm_stats_tiles(int Nb, int OH, int OW);
int dasac_conv_gemm_stats(const float* x, const float* packed, const int32_t* table, float* out,
                          int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                          int OutH, int OutW, int ostride, const float* shift, const float* res, int relu,
                          int pix_begin, int pix_count, int schedule, void* workspace, size_t ws_bytes,
                          float* stats, dasac_stream_t stream);
size_t dasac_conv_gemm_workspace(void);
int dasac_conv_gemm_schedule(int Nb, int OH, int OW, int M, int K);   /* 1 = stream-K, 0 = one block per tile */
/* > 0: dasac_conv_gemm(schedule 0, the whole pixel range, workspace given) runs this shape as ONE launch -- the leading whole
 * rounds of resident workgroups one block per tile, the remaining tiles cut into that many K-ranges of one block each (split-K
 * tail: the later ranges deposit their accumulators in the workspace, the piece with the first K-steps adds them and runs
 * the epilogue; deterministic: a function of the shape and the reserved CUs alone).  0: it does not. */
int dasac_conv_gemm_tail_split(int Nb, int OH, int OW, int M, int K);
size_t dasac_conv_wgrad_workspace(int Nb, int OH, int OW, int M, int K);
int dasac_conv_wgrad(const float* dz, const float* x, const int32_t* table,
                     int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                     void* workspace, size_t ws_bytes, dasac_stream_t stream);
/* split-bf16 variant of dasac_conv_wgrad (same arguments, workspace layout and dasac_conv_wgrad_finish):
 * both operands are split on their way into LDS, three bf16 MFMAs per product, fp32 accumulate. */
int dasac_conv_wgrad_x3(const float* dz, const float* x, const int32_t* table,
                        int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int K,
                        void* workspace, size_t ws_bytes, dasac_stream_t stream);
int dasac_conv_wgrad_dot_rows(int Cin, int taps);
int dasac_conv_wgrad_finish(const void* workspace, int Nb, int OH, int OW, int M, int K,
                            const float* w, const float* scale, float* dw, float* dot,
                            float* sum_dz, int Cin, int taps, int tap0, dasac_stream_t stream);

/* Winograd F(2x2,3x3) evaluation of 3x3, stride-1 convolutions with padding == dilation (the 512 -> 512, dilation-4 conv2 of the
 * layer4 bottlenecks, deeplabv2.py:65-66), forward and data gradient: 2.25 x fewer multiplies than the direct contraction, UNFUSED --
 * three streaming kernels around ONE batched launch of the 16 point GEMMs (dasac_conv_gemm_batched), no matrix kernel of its own.  The d*d dilation phases of the map
 * are cut into 2x2-output tiles; T = dasac_winograd_tiles(Nb, H, W, dilation) of them in all (tile numbering: csrc/winograd_index.hpp).
 *   dasac_winograd_filter  u = 16 packed matrices, one per Winograd point pt = 4a + b, each laid out as dasac_conv_pack lays out a
 *                          1x1 convolution (dasac_conv_kpad(K) * dasac_conv_mpad(M) floats per point, padding written as zeros):
 *                          U[pt] = (G g G^T)[a][b] with g = w[co][ci] * scale[co] (scale may be NULL).  transposed = 0: M = Cout,
 *                          K = Cin (forward); transposed = 1: M = Cin, K = Cout and g rotated by 180 degrees (data gradient).
 *   dasac_winograd_input   v [16][C][T] = B^T d B of every tile's 4x4 patch of x [Nb,C,H,W] (taps `dilation` apart, zero outside
 *                          the image).  v_bytes >= 16*C*T*4.
 *   point GEMMs (caller)   dasac_conv_gemm_batched(x = v, packed = u, table of a 1x1 convolution over planes of 1 x T, out = y,
 *                          Nb = 1, Cx = K = C, H = OH = 1, W = OW = T, batch = 16, strides C*T, Kpad*Mpad, M*T) -- or, bit for bit
 *                          the same, for pt in 0..15: dasac_conv_gemm on the pt-th slices, no epilogue operands
 *   dasac_winograd_output  out [Nb,M,H,W] = epi(A^T Y A): + shift[m] (may be NULL), ReLU when `relu`; relu_bits_out (relu = 1)
 *                          receives the pattern out > 0 and mask_bits zeroes the elements whose bit is clear, both in the layout of
 *                          dasac_conv_gemm's bit masks (dasac_relu_bits_words(M, Nb*H*W) words); at most one of the two.
 *                          Tiles that hang over the map edge store their in-image pixels only.  y_bytes >= 16*M*T*4.
 * Rounding differs from the direct contraction (two transforms of additions in front of and behind the products): within a small
 * multiple of its error against an exact convolution, not bit-equal to it. */
int dasac_winograd_tiles(int Nb, int H, int W, int dilation);
int dasac_winograd_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                          dasac_stream_t stream);
int dasac_winograd_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                         dasac_stream_t stream);
int dasac_winograd_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                          int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out, dasac_stream_t stream);
/* Weight gradient of the same convolutions in the same form, the exact adjoint of the forward path:
 * dW = G^T [ sum over tiles of (A dY A^T) (.) (B^T x B) ] G, 2.25 x fewer multiplies than dasac_conv_wgrad.
 *   dasac_winograd_input        v [16][C][T] = B^T d B of x, as in the forward pass (recomputed: nothing is kept from it)
 *   dasac_winograd_grad_input   dm [16][M][T] = (A dY A^T)[pt] of every tile's 2x2 output pixels of dz [Nb,M,H,W], A = [[1,0],[1,1],
 *                               [1,-1],[0,-1]], tiles numbered as dasac_winograd_input numbers them; a pixel of a tile that hangs
 *                               over the map edge counts as zero.  dm_bytes >= 16*M*T*4.
 *   dasac_conv_wgrad_batched    `batch` weight gradients over plain row-major matrices as ONE launch (grid y = batch entry):
 *                               P[split][b][m][c] = sum over the split's t of a[b][m][t] * b[b][c][t], entries a_stride / b_stride
 *                               ELEMENTS apart, slabs in `workspace` (dasac_conv_wgrad_batched_workspace bytes), followed by
 *                               Psum[split][m] = the split's row sums of entry `sum_entry` of a.  The pixel splits
 *                               (dasac_conv_wgrad_batched_splits; 0 = shape not taken) are chosen over all batch * M/128 * C/128
 *                               tiles.  Fixed summation order, no atomics: the bits repeat from run to run.  Needs batch in
 *                               1..65535, M and C multiples of 128, T a multiple of 4, strides >= one entry's extent (M*T, C*T)
 *                               and multiples of 4 elements, an entry below 2 GiB and the slabs inside the 4 GiB window; anything
 *                               else is DASAC_EINVAL.  The Winograd weight gradient calls it with a = dm, b = v, batch = 16 and
 *                               sum_entry = 5: point (1,1) of A dY A^T is the tile's pixel sum, so its row sums are sum dz.
 *   dasac_winograd_wgrad_finish adds the splits in a fixed order, applies G^T (.) G and writes dw[co][ci][3][3] = scale[co] * gradient
 *                               (scale may be NULL); dot (may be NULL) [C/64][M] and sum_dz (may be NULL) [M] are what
 *                               dasac_conv_wgrad_finish leaves there: per block of 64 input channels the partial sum of w * (unscaled
 *                               gradient), and the sum of dz over batch and pixels.  M = Cout, C = Cin (a multiple of 64). */
int dasac_winograd_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                              dasac_stream_t stream);
int dasac_conv_wgrad_batched_splits(int batch, int M, int C, int T);
size_t dasac_conv_wgrad_batched_workspace(int batch, int M, int C, int T);
int dasac_conv_wgrad_batched(const float* a, const float* b, int batch, int M, int C, int T, int64_t a_stride, int64_t b_stride,
                             int sum_entry, void* workspace, size_t ws_bytes, dasac_stream_t stream);
int dasac_winograd_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w, const float* scale,
                                float* dw, float* dot, float* sum_dz, dasac_stream_t stream);
/* The same weight gradient as Winograd F(4x4,3x3), evaluation points 0, 1, -1, 2, -1/2, inf: 36 point products per 4x4-output tile,
 * 1.71 x fewer multiplies than the F(2x2) form on large maps, at a few times its rounding error (a weight gradient is a terminal
 * sum; the forward and the data gradient in this form follow below).  The phases are cut into 4x4-output tiles, and
 * T = dasac_winograd4_tiles(Nb, H, W, dilation) is their count ROUNDED UP to a multiple of 4 (what dasac_conv_wgrad_batched needs);
 * both transforms write the padding tiles as zeros at all 36 points.
 *   dasac_winograd4_input        v [36][C][T] = B^T d B of every tile's 6x6 patch of x.  v_bytes >= 36*C*T*4.
 *   dasac_winograd4_grad_input   dm [36][M][T] = A dY A^T of every tile's 4x4 output pixels of dz.  dm_bytes >= 36*M*T*4.
 *   dasac_conv_wgrad_batched     batch = 36, strides M*T and C*T, sum_entry = 7: point (1,1), evaluation point 1 on both axes, is
 *                                the tile's pixel sum.
 *   dasac_winograd4_wgrad_finish as dasac_winograd_wgrad_finish over the 36 slabs per split
 *                                (ws_bytes >= dasac_conv_wgrad_batched_workspace(36, M, C, T)), G^T (.) G from 6x6 to 3x3. */
int dasac_winograd4_tiles(int Nb, int H, int W, int dilation);
int dasac_winograd4_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                          dasac_stream_t stream);
int dasac_winograd4_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                               dasac_stream_t stream);
int dasac_winograd4_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w, const float* scale,
                                 float* dw, float* dot, float* sum_dz, dasac_stream_t stream);
/* Forward and data gradient of the same convolutions as F(4x4,3x3), same points: 36 products per 16 outputs where F(2x2) spends 64,
 * at 2 - 4 x the direct kernel's rounding error.  The twins of the F(2x2) entry points around dasac_winograd4_input (x in the
 * forward, dz in the data gradient) and ONE dasac_conv_gemm_batched launch of 36 entries (strides C*T, Kpad*Mpad, M*T):
 *   dasac_winograd4_filter  u = 36 packed matrices, point pt = 6a + b, U[pt] = (G g G^T)[a][b]; modes as dasac_winograd_filter.
 *   dasac_winograd4_output  out [Nb,M,H,W] = epi(A^T Y A) of y [36][M][T], epilogue operands as dasac_winograd_output.  The padding
 *                           tiles and the outputs of a tile that hang over the map edge store nothing.  relu_bits_out is packed
 *                           from the stored output by a second launch (the transform's lanes run along tiles, not pixels: no
 *                           ballot), every word written.  y_bytes >= 36*M*T*4. */
int dasac_winograd4_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                           dasac_stream_t stream);
int dasac_winograd4_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                           int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out, dasac_stream_t stream);

/* Tap-expanded evaluation of few-output-channel, many-tap convolutions -- the ASPP classifiers
 * (deeplabv2.py:101-116): Y[(tap,co)] = 1x1 GEMM over taps*Cp channels (dasac_conv_gemm with weights
 * from dasac_conv_pack_expanded), out = bias + sum_tap shift(Y) (dasac_tap_gather); backward:
 * D = dasac_tap_scatter(dout), then plain 1x1 wgrad / dgrad on D.  Cp >= Cout pads the channels so
 * that taps*Cp % 16 == 0.  Branches are (kh,kw,dilation,padding) as for dasac_conv_table. */
int dasac_conv_pack_expanded(const float* w, int Cout, int Cin, int taps, int tap0, int total_taps,
                             int Cp, int transposed, float* packed, dasac_stream_t stream);
int dasac_tap_gather(const float* y, const int32_t* kh, const int32_t* kw, const int32_t* dil,
                     const int32_t* pad, int n_branches, int Cp, int Cout, const float* bias, int B,
                     int H, int W, float* out, dasac_stream_t stream);
int dasac_tap_scatter(const float* dout, const int32_t* kh, const int32_t* kw, const int32_t* dil,
                      const int32_t* pad, int n_branches, int Cp, int Cout, int B, int H, int W,
                      float* d, dasac_stream_t stream);
int dasac_conv_wgrad_finish_expanded(const void* workspace, int Nb, int OH, int OW, int E, int Cin,
                                     float* dw, int Cout, int taps, int tap0, int Cp,
                                     dasac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SAC head (models/sac.py) -- HBM-bound streaming kernels over [B,C,H,W] fp32, C <= 32.
 *
 * dasac_upsample_softmax  F.interpolate(bilinear, align_corners=True) of logits [B,C,h,w]
 *     (deeplabv2.py:217, sac.py:275); optional outputs: `up` (upsampled logits), `probs` =
 *     softmax zeroed where ignore != 0 (sac.py:276,282), `class_sums[C]` (double) = sum over
 *     batch and pixels of the unmasked softmax (sac.py:108), accumulated order-independently (Q32 fixed point,
 *     B*H*W < 2^31) so that the class prior is bit-identical from run to run.
 * dasac_upsample_bwd      transpose of the upsampling: grad_low = gscale[0] * U^T grad_up
 *     (gscale: device scalar or NULL), planes = B*C.
 * dasac_ce_loss           mode 0: mean over ALL pixels of CE(ignore 255) (deeplabv2.py:223-224,
 *     sac.py:119-132); mode 1: focal_ce_conf with its [B,B,H,W] broadcast (sac.py:134-149):
 *     loss = sum_hw (sum_i conf_i)(sum_j ce_j)/(B*B*HW).  class_weight [C] or NULL.  dlogits
 *     (optional) receives gscale[0] * d loss / d logits (gscale: device scalar = upstream
 *     gradient of the loss, NULL = 1); per_class (optional) [C] as sac.py:138-145 (order-independent Q28 fixed-point
 *     accumulation: per-pixel values are clamped to |ce| <= 4096 there; the loss itself is not clamped).
 *     Labels: 255 is the ignore index, and EVERY label outside [0, C) is treated like it (F.cross_entropy raises on
 *     those): such a pixel carries no loss, no gradient (its dlogits are exactly 0) and no per_class term, but still
 *     counts in the mean's divisor.  dasac_ce_loss_bwd_low follows the same rule.
 * dasac_warp_affine       grid_sample(x, affine_grid(theta), bilinear, zeros, align_corners=False)
 * dasac_warp_pool         sac.py:289-305 with _avg_pool (mode 0, :238-269) or _minentropy_pool
 *     (mode 1, :218-236): probs [N*T,C,H,W] -> pooled [N,C,H,W], mask [N,H,W]; `aligned`
 *     (optional) = teacher_aligned diagnostic [N*T,C,H,W].  theta == theta_inv == NULL: `probs` are
 *     views that are already aligned and coverage-weighted (the pooling functions on their own).
 * dasac_warp_back         sac.py:309-311: refined[b] = warp(pooled[b/views_per_group]) * warp(mask); any H, W >= 1 (W >= 2
 *     fetches the two taps of a source row as one 8-byte pair, one-column maps take four scalar taps: the same arithmetic)
 * dasac_class_state       sac.py:104-117 running prior update (if update) and the derived
 *     vectors disc = 1-exp(-chi/beta) (:152), focal = (1-max(chi,0))^p (:120); any may be NULL.
 */
int dasac_upsample_softmax(const float* logits, int B, int C, int h, int w, int H, int W,
                           const uint8_t* ignore, float* up, float* probs, double* class_sums,
                           dasac_stream_t stream);
size_t dasac_upsample_bwd_workspace(int planes, int H, int w);
int dasac_upsample_bwd(const float* grad_up, int planes, int h, int w, int H, int W,
                       const float* gscale, float* grad_low, void* workspace, size_t ws_bytes,
                       dasac_stream_t stream);
size_t dasac_ce_loss_workspace(int B, int C, int64_t HW);
int dasac_ce_loss(const float* logits, const int64_t* labels, const float* class_weight,
                  const float* conf, int B, int C, int64_t HW, int mode, const float* gscale,
                  float* loss, float* dlogits, float* per_class, void* workspace, size_t ws_bytes,
                  dasac_stream_t stream);
/* Gradient of dasac_ce_loss w.r.t. the LOW-resolution logits the upsampled ones came from (deeplabv2.py:217 then
 * :223-224 / sac.py:119-149): grad_low [B,C,h,w] = gscale[0] * U^T (d loss / d logits_up) without materialising the
 * full-resolution gradient (same arithmetic and summation order as dasac_ce_loss(dlogits) + dasac_upsample_bwd).
 * The workspace holds the row buffer [B*C][H][w] and, behind it, H*W floats for the per-pixel confidence sums of mode 1
 * (added up once per launch instead of once per image; the size function reserves H*w*16 floats = any up-factor to 16; a
 * workspace with only the row buffer still works, every block then adds the B confidences itself). */
size_t dasac_ce_loss_bwd_low_workspace(int B, int C, int H, int w);
int dasac_ce_loss_bwd_low(const float* logits_up, const int64_t* labels, const float* class_weight, const float* conf,
                          int B, int C, int H, int W, int h, int w, int mode, const float* gscale, float* grad_low,
                          void* workspace, size_t ws_bytes, dasac_stream_t stream);
/* Inference (infer_val.py:160-163 and the result writer's argmax + trainId->labelId mapping, :60-65):
 * labels[b,y,x] = lut[argmax_c softmax(bilinear_ac(logits))[b,c,y,x]] (lut null: the class index), optional
 * conf = the winning probability.  1 (+4) bytes written per output pixel. */
int dasac_infer_labels(const float* logits, int B, int C, int h, int w, int H, int W, const uint8_t* lut,
                       uint8_t* labels, float* conf, dasac_stream_t stream);
/* Test-time augmentation around it (infer_val.py is single-scale; the usual evaluation form runs the image at a few scales,
 * plain and mirrored, and averages the class probabilities).
 * dasac_image_pyramid  out[0:B] = F.interpolate(image [B,Cin,H,W], (Hs, Ws), bilinear, align_corners=True); with_flip: out is
 *     [2B,Cin,Hs,Ws] and out[B:2B] = out[0:B].flip(-1), bit for bit (the same thread writes both: one read of the source).
 *     The source coordinate dst*(n_in-1)/(n_out-1) is taken in integers (quotient = tap, remainder/(n_out-1) = weight), so the
 *     result is within fp32 rounding of the float64 interpolate at any scale.  Hs*H and Ws*W < 2^31.
 *     Hs == H && Ws == W is legal: the weights are exactly (1, 0) and out[0:B] == image.  B*Cin < 65536.
 * dasac_infer_fuse     dasac_infer_labels over n_sources <= DASAC_INFER_MAX_SOURCES logit tensors [B,C,h_s,w_s] in ONE pass
 *     per output pixel:  p_s = softmax_c(bilinear_ac(logits_s))[b,:,y, flip_s ? W-1-x : x]  (= interpolate(.).flip(-1) for a
 *     source computed from the mirrored image), same arithmetic per source as dasac_infer_labels;
 *     fused = (p_0 + p_1 + ...) * (1.f / n) in source order (DASAC_INFER_MEAN) or max_s p_s (DASAC_INFER_MAX);
 *     labels u8 [B,H,W] = lut[argmax_c fused] (first maximum wins; lut NULL: the class index), conf f32 [B,H,W] (optional) = the
 *     winning fused value, probs f32 [B,C,H,W] (optional) = all of them (what infer_val.py's D_SAVE_RAW stores).
 *     `sources` is a HOST array; its records travel to the kernel by value: no device table, no workspace.  Both entries run
 *     the same kernel: dasac_infer_labels is one unflipped source.  C <= 32.  1 (+4) (+4C) bytes written per output pixel. */
#define DASAC_INFER_MAX_SOURCES 8
#define DASAC_INFER_MEAN 0
#define DASAC_INFER_MAX 1
typedef struct dasac_infer_source {
  const float* logits; /* device, [B,C,h,w] */
  int32_t h, w, flip, reserved;
} dasac_infer_source;
int dasac_image_pyramid(const float* image, int B, int Cin, int H, int W, int Hs, int Ws, int with_flip, float* out,
                        dasac_stream_t stream);
int dasac_infer_fuse(const dasac_infer_source* sources, int n_sources, int B, int C, int H, int W, int mode,
                     const uint8_t* lut, uint8_t* labels, float* conf, float* probs, dasac_stream_t stream);
int dasac_warp_affine(const float* x, const float* theta, int B, int C, int H, int W, float* out,
                      dasac_stream_t stream);
int dasac_warp_pool(const float* probs, const float* theta, const float* theta_inv, int N, int T,
                    int C, int H, int W, int mode, float tolerance, float* aligned, float* pooled,
                    float* mask, dasac_stream_t stream);
int dasac_warp_back(const float* pooled, const float* mask, const float* theta_inv, int B,
                    int views_per_group, int C, int H, int W, float* refined,
                    dasac_stream_t stream);
int dasac_class_state(float* running_conf, const double* class_sums, int B, int64_t HW, int C,
                      float beta, float stat_momentum, int update, float focal_p, float* disc,
                      float* focal, dasac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Around the convolutions.
 * dasac_bn_fold          frozen BatchNorm (models/__init__.py:29, basenet.py:97-100) as per-channel
 *     scale/shift for the conv epilogue: scale = gamma/sqrt(var+eps), shift = beta-(mean-b)*scale.
 *     `conv_bias` (b, NULL = no bias) and `invstd` (NULL = not wanted) are optional; every other pointer is required.
 * dasac_bn_param_grads   gamma/beta (and conv-bias) gradients of the folded form from
 *     sum_rows dot[row][c] = sum dz*conv(x) (the `dot_rows` partial rows of dasac_conv_wgrad_finish) and sum_dz[c]
 *     (dasac_channel_sums or the wgrad kernel): dgamma = invstd*(dot + (b - mean)*sum_dz), dbeta = sum_dz,
 *     dbias = scale*sum_dz.  Each of dgamma / dbeta / dbias may be NULL and is then not written; `dot`, `mean` and `invstd`
 *     are read only for dgamma (dgamma without them is DASAC_EINVAL); `scale` NULL = 1, `conv_bias` NULL = 0.
 * dasac_maxpool_fwd/bwd  nn.MaxPool2d (deeplabv2.py:126 ceil_mode 3x3/2; VGG 2x2/2); caller passes
 *     the resolved OH/OW.  bwd with relu_mask folds the ReLU backward of the producer.  `argmax` is an opaque byte per
 *     output handed from fwd to bwd: bits 0-6 the winning position kh*k + kw, bit 7 (windows up to 11x11) = pooled value > 0,
 *     so that the ReLU-folding backward does not read the pooled tensor (`y` is then unused; larger windows do read it).
 * dasac_ema_update       momentum teacher (sac.py:83-102) over all tensors in one launch:
 *     out[0] = sum_t ||slow_t - fast_t||_2 (before the update); slow = slow*m + fast*(1-m): three fp32 roundings with
 *     the factors fl32(m) and fl32(1 - m), the difference taken in double as sac.py:95 takes it (hence `double momentum`).
 *     update = 0 writes no slow tensor; out[0] is the same distance either way.
 *     `pairs`: device array of {const float* fast; float* slow; int64 n}; `chunks`: device (tensor, chunk) int32 pairs of
 *     dasac_ema_chunk_elems() elements, SORTED by tensor; `sq`: scratch of n_tensors + n_chunks doubles (one partial per
 *     chunk, added per tensor in a fixed order: the result is bit-identical from run to run).  `pairs`, `chunks` and `sq`
 *     must be 8-byte aligned (64-bit fields, int32 pairs read as one word); the tensors they point to need element alignment.
 * dasac_scale_planes     Dropout2d with an explicit per-(n,c) keep mask (fcn.py:52,56).
 */
int dasac_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                  const float* conv_bias, float eps, int C, float* scale, float* shift,
                  float* invstd, dasac_stream_t stream);
int dasac_bn_param_grads(const float* dot, int dot_rows, const float* sum_dz, const float* mean,
                         const float* invstd, const float* scale, const float* conv_bias, int C,
                         float* dgamma, float* dbeta, float* dbias, dasac_stream_t stream);
int dasac_channel_sums(const float* x, int N, int C, int64_t HW, float* out, dasac_stream_t stream);
int dasac_maxpool_fwd(const float* x, int planes, int H, int W, int OH, int OW, int k, int s,
                      int pad, float* y, uint8_t* argmax, dasac_stream_t stream);
int dasac_maxpool_bwd(const float* dy, const float* y, const uint8_t* argmax, int planes, int H,
                      int W, int OH, int OW, int k, int s, int pad, int relu_mask, float* dx,
                      dasac_stream_t stream);
int dasac_ema_chunk_elems(void);
/* torch.optim.SGD(momentum, no nesterov, dampening 0) over all parameters of up to 8 groups in ONE launch
 * (base_trainer.py:63-66 over basenet.py:73-95):  d = g + wd*p; buf = first ? d : momentum*buf + d; p -= lr*buf.
 * tensors: device array of {float* p; const float* g; const float* g2 (NULL or a second gradient, summed as g2 + g before
 * anything else -- what two backward passes would have accumulated into .grad); float* buf; int64 n; int64 group}; chunks as for
 * dasac_ema_update ((tensor, chunk) pairs of dasac_ema_chunk_elems() elements); group_lr/group_wd: HOST arrays.
 * `tensors` and `chunks` must be 8-byte aligned, here and in dasac_sgd_nesterov_step, dasac_adam_step, dasac_grad_norm and the
 * _ctl forms; p, g, g2 and the state tensors may lie at any 4-byte phase (the bits do not depend on it). */
int dasac_sgd_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                   const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                   dasac_stream_t stream);
/* The same with Nesterov momentum (OPT_NESTEROV, base_trainer.py:64; torch/optim/sgd.py:462-473): buf as above, then
 * p -= lr*(d + momentum*buf).  Table, chunks, group arrays and the `first` split are those of dasac_sgd_step; momentum > 0. */
int dasac_sgd_nesterov_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                            const float* group_lr, const float* group_wd, int n_groups, float momentum,
                            int first, dasac_stream_t stream);
/* torch.optim.Adam (OPT: Adam, base_trainer.py:57-61 with betas = (BETA1, 0.999), core/config.py:135-140: BETA1 = 0.5) over all
 * parameters of up to 8 groups in ONE launch: L2 weight decay in the gradient, no amsgrad, no maximize, not decoupled.  Per
 * element, in the operation order of torch/optim/adam.py:689-800 (foreach, not capturable):
 *   g = (g2 +) g (+ wd*p);  m = lerp(m, g, 1 - beta1) (ATen's two-branch lerp, Lerp.h:32-34);  v = v*beta2 + (1 - beta2)*(g*g);
 *   p += -step_size * (m / (sqrt(v)/bc2_sqrt + eps)).
 * tensors: device array of 64-byte rows {float* p; const float* g; const float* g2 (NULL or a second gradient, as for
 * dasac_sgd_step); float* exp_avg; float* exp_avg_sq; int64 n; int32 group; int32 reserved; float step_size; float bc2_sqrt}
 * with step_size = lr/(1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) of THAT tensor's step count, computed by the caller
 * in doubles as adam.py:772-781 does and rounded to fp32.  chunks as for dasac_ema_update; group_wd: HOST array.  1 - beta1
 * and 1 - beta2 are formed in double here and rounded to fp32 once, as the foreach kernels receive them. */
int dasac_adam_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                    const float* group_wd, int n_groups, double beta1, double beta2, double eps,
                    dasac_stream_t stream);
/* Global L2 gradient-norm clipping and non-finite step skipping for the three updates above, without a host synchronisation.
 * dasac_grad_norm reads g, g2 and n from the SAME uploaded table the update reads (row_bytes names it: 48 = the rows of
 * dasac_sgd_step, 64 = those of dasac_adam_step) over the same chunks, and writes the 16-byte device control block
 *   ctl = {float total; float coef; int32 skip; int32 reserved}
 *   total = (float)sqrt(sum over all elements of (g2 + g)^2): the fp32 sum the update applies, squared and added in double, one
 *           partial per chunk in `workspace` (dasac_grad_norm_workspace(n_chunks) bytes), no atomics, partials added in a fixed
 *           order: the same inputs give the same bits, wherever the gradients lie (16-byte loads or not);
 *   coef  = min(max_norm / (total + 1e-6f), 1.0f) in fp32 as torch.nn.utils.clip_grad_norm_ forms it (NaN stays NaN), or
 *           1.0f with max_norm <= 0 (measure only);
 *   skip  = total is not finite.
 * `skipped` (NULL, or a device int64 counter) grows by `skip`.  ctl must be 16-byte aligned.
 * The _ctl updates are the plain ones plus: apply_coef = 1 multiplies the summed gradient by ctl->coef (one fp32 multiply,
 * before weight decay); honour_skip = 1 makes the launch write nothing while ctl->skip is set -- except that a FIRST SGD step
 * writes buf = -0, so that the next step's momentum*buf + d is the first-step rule without the host knowing.  The SGD forms
 * also take first = -1: bit 32 of each row's `group` then says whether that tensor takes its first step (one table, hence
 * one norm, for a step in which some tensors are new); `group` itself is bits 0-2. */
size_t dasac_grad_norm_workspace(int n_chunks);
int dasac_grad_norm(const void* tensors, int row_bytes, int n_tensors, const int32_t* chunks, int n_chunks,
                    float max_norm, void* workspace, size_t workspace_bytes, void* ctl, int64_t* skipped,
                    dasac_stream_t stream);
int dasac_sgd_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                       const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                       const void* ctl, int apply_coef, int honour_skip, dasac_stream_t stream);
int dasac_sgd_nesterov_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                const float* group_lr, const float* group_wd, int n_groups, float momentum,
                                int first, const void* ctl, int apply_coef, int honour_skip, dasac_stream_t stream);
int dasac_adam_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                        const float* group_wd, int n_groups, double beta1, double beta2, double eps,
                        const void* ctl, int apply_coef, int honour_skip, dasac_stream_t stream);
/* Per-tensor gradient health table: one more pass over the SAME uploaded table and chunks as dasac_grad_norm (row_bytes 48 or
 * 64), which also reads p at byte 0 and the state pointer at byte 24 (momentum_buffer / exp_avg); either may be NULL and then
 * gives zeros in its columns.  table: n_rows x 8 doubles, row r describing tensor row_of[r] of `tensors` (a device int32 array;
 * -1, a parameter with nothing pending: eight zeros), d = g2 + g being the fp32 sum the update applies:
 *   0 g_sumsq   sum d^2 over finite d        1 g_maxabs  max |d| over finite d       2 g_nonfinite  number of Inf / NaN d
 *   3 g_first_nonfinite  1 + flat index of the first non-finite d, 0 if none          4 g_zeros      number of d == 0
 *   5 p_sumsq   sum p^2 (Inf / NaN show)     6 p_maxabs  max |p| over finite p       7 s_sumsq      sum state^2
 * One partial row per chunk in `workspace` (dasac_tensor_stats_workspace(n_chunks) bytes), no atomics, partials combined in a
 * fixed order: the same inputs give the same bits, wherever the tensors lie.
 * PRECONDITION: `chunks` is ordered by tensor (every tensor's chunks form one contiguous run, tensor ids ascending), as for
 * dasac_ema_update: the rows are found by binary search.
 * FIRST STEP: in the 48-byte table a row with bit 32 of `group` set takes its first step (dasac_sgd_step_ctl, first = -1); its
 * momentum buffer is uninitialised and is not read: s_sumsq = 0.
 * ctl, captured, captured_at and skipped are all NULL (measure only) or all given: while ctl->skip is set (dasac_grad_norm on
 * the same stream, before this call) the table is also written to `captured` (n_rows x 8 doubles) and *captured_at = *skipped. */
size_t dasac_tensor_stats_workspace(int n_chunks);
int dasac_tensor_stats(const void* tensors, int row_bytes, int n_tensors, const int32_t* chunks, int n_chunks,
                       const int32_t* row_of, int n_rows, void* workspace, size_t workspace_bytes, double* table,
                       const void* ctl, double* captured, int64_t* captured_at, const int64_t* skipped,
                       dasac_stream_t stream);
/* Per-layer activation health / domain-gap table: one streaming pass over fp32 activations [N, C, H*W] that a forward pass
 * already holds, reduced per channel and per sample segment.  `tensors`: a device array of n_tensors 32-byte rows
 *   { const float* x; int64_t HW; int32_t C; int32_t row0; int64_t plane0; }
 * each one contiguous tensor [N, C, HW], 1 <= HW <= 2^30 (a row outside that gives zeros); row0 / plane0 are the prefix sums of C / N*C over the earlier rows (row 0 has 0, 0), all
 * tensors of a call share N, R = sum C is the number of channel rows and N*R the number of planes.  The rows live in device
 * memory, so R is passed beside them: it sizes both grids and the workspace check.  `seg_bounds`: a device array of
 * n_segments + 1 sample indices, strictly ascending from 0 to N, 1 <= n_segments <= 8; segment s covers samples
 * seg_bounds[s] .. seg_bounds[s+1]-1 (device memory: the caller vouches for it; the kernel clamps what it reads to 0..N).
 * table: [n_segments][R][6] doubles; for segment s and channel c of tensor t (row row0_t + c), over that segment's samples:
 *   0 sum     sum x over finite x, each widened to double    3 nonfinite        number of Inf / NaN entries
 *   1 sumsq   sum x^2 over finite x, squared in double       4 first_nonfinite  1 + flat NCHW index IN ITS TENSOR of the first
 *   2 maxabs  max |x| over finite x, 0 if none                                  non-finite entry of the segment, 0 if none
 *                                                            5 zeros            number of x == 0 (either sign)
 * One 256-thread block per (tensor, sample, channel) plane writes one partial row to `workspace`
 * (dasac_activation_stats_workspace(N*R) bytes); one wave per (segment, row) adds the segment's samples in ascending order.  No
 * atomics, every combination in a fixed order, and an element's owner thread and a thread's summation order depend on the
 * element's index inside its plane, never on its address: the same values give the same bits wherever each tensor lies (planes
 * of 97 x 97 or 769 x 769 floats start on every 4-byte phase).  Bad arguments (null pointers; n_tensors, N, R or n_segments out
 * of range; workspace too small) return DASAC_EINVAL before any launch and leave `table` untouched. */
size_t dasac_activation_stats_workspace(int64_t n_planes);
int dasac_activation_stats(const void* tensors, int n_tensors, int N, int R, const int32_t* seg_bounds, int n_segments,
                           void* workspace, size_t workspace_bytes, double* table, dasac_stream_t stream);
/* Class-conditional feature tables: the moments of an activation per CLASS and channel, the class of a position taken from a
 * label map brought to the feature map's own resolution.
 * dasac_label_nodes  labels [N,H,W] int64 or uint8 (labels_u8), as the count kernels take them -> nodes u8 [N,h,w].  Node (i,j)
 *     sits where align_corners=True upsampling puts it: pixel (Y(i), X(j)), Y(i) = (2*i*(H-1) + (h-1)) / (2*(h-1)) in integers
 *     (halves round up; 0 when h == 1), X likewise.  nodes[n,i,j] = v, the label at that pixel, if 0 <= v < C and every pixel of
 *     the window [Y-radius, Y+radius] x [X-radius, X+radius], clipped to the image, holds v; 255 otherwise.  So 255, -1 and any
 *     value >= C leave their own node and every node whose window touches them without a class.  radius 0..8 (0: nearest
 *     sampling), C 1..255.  Keeps prototypes to region interiors: a stride-8 feature at a contour is a mixture.
 * dasac_class_feature_stats  x [N,Cf,HW] fp32, nodes [N,HW] u8 (any byte address).  For every class c < C <= 32 and channel f,
 *     over all (n,p) with nodes[n,p] == c:  sums[c][f][0] += sum x,  sums[c][f][1] += sum x^2  (each x widened to double, squared
 *     in double),  counts[c] += their number.  sums: double [C][Cf][2], counts: int64 [C]; both ACCUMULATE -- the caller
 *     zero-fills them once and a loader's batches add up.  A node >= C belongs to no class.  There is no finite filter: a
 *     non-finite x makes its cell non-finite (dasac_activation_stats finds those).  One 256-thread block per (sample, group of
 *     channels) writes one partial row [C][2] per (sample, channel) to `workspace` (dasac_class_feature_stats_workspace =
 *     N*Cf*C*16 bytes, 8-byte aligned); one lane per (channel, class) adds the samples in ascending order and then adds the
 *     result to sums.  No floating-point atomics, every combination in a fixed order, and an element's owner thread and a
 *     thread's summation order depend on the element's index inside its plane, never on its address: the same values give the
 *     same bits wherever x and nodes lie.  counts uses integer adds (exact in any order).  Bad arguments (null pointers, C
 *     outside 1..32, N outside 1..65535, HW outside 1..2^30-1, workspace too small) return DASAC_EINVAL before any launch and
 *     leave sums and counts untouched. */
int dasac_label_nodes(const void* labels, int labels_u8, int N, int H, int W, int h, int w, int C, int radius,
                      uint8_t* nodes, dasac_stream_t stream);
size_t dasac_class_feature_stats_workspace(int N, int Cf, int C);
int dasac_class_feature_stats(const float* x, const uint8_t* nodes, int N, int Cf, int HW, int C,
                              double* sums, int64_t* counts, void* workspace, size_t ws_bytes, dasac_stream_t stream);
int dasac_ema_update(const void* pairs, int n_tensors, const int32_t* chunks, int n_chunks,
                     double momentum, int update, double* sq, float* out, dasac_stream_t stream);
int dasac_scale_planes(const float* x, const float* plane_scale, int64_t planes, int64_t HW,
                       float* y, dasac_stream_t stream);
int dasac_add(const float* a, const float* b, float* out, int64_t n, dasac_stream_t stream);
/* out = y > 0 ? dy : 0  (ReLU backward, F.relu / nn.ReLU(inplace) of deeplabv2.py:84,88,97) */
int dasac_relu_mask(const float* dy, const float* y, float* out, int64_t n, dasac_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode BatchNorm (baseline / AdaBN mode, models/__init__.py:29; nn.SyncBatchNorm of
 * deeplabv2.py:15, fcn.py:8; running-stat re-estimation of train.py:281-289).
 * Both reductions are two-stage and atomic-free (one partial pair per plane and 4096-element chunk in `workspace` of
 * dasac_bn_stats_workspace(N, C, HW) bytes, then a fixed-order sum per channel): bit-identical from run to run.
 * forward:  dasac_bn_stats (sums[0:C] = sum z, sums[C:2C] = sum z^2, doubles) -> [caller all-reduces
 *           `sums` and the element count across ranks = SyncBN] -> dasac_bn_train_finalize (batch
 *           mean / biased var -> scale, shift, mean, invstd; running stats updated with momentum and
 *           the unbiased var; running_* may be NULL) -> dasac_bn_apply (y = relu?(z*scale+shift(+res))).
 * backward: dasac_bn_bwd_reduce (sums = sum dy, sum dy*xhat) -> [all-reduce] -> dasac_bn_bwd_apply
 *           (dz = gamma*invstd*(dy - sum_dy/n - xhat*sum_dy_xhat/n); dgamma, dbeta optional).
 * `count` = elements per channel over all ranks; `count_dev` (device double, may be NULL) overrides it so
 * that an all-reduced count never has to visit the host.
 */
size_t dasac_bn_stats_workspace(int N, int C, int64_t HW);
int dasac_bn_stats(const float* z, int N, int C, int64_t HW, double* sums, void* workspace, size_t ws_bytes,
                   dasac_stream_t stream);
int dasac_bn_train_finalize(const double* sums, double count, const double* count_dev, const float* gamma,
                            const float* beta, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked /* += 1 when given */, float momentum, float eps, int C,
                            float* scale, float* shift, float* mean, float* invstd,
                            dasac_stream_t stream);
/* The same with the statistics left by dasac_conv_gemm_stats: dasac_bn_train_finalize_tiles sums the tiles itself (one launch
 * per BN layer on one rank); dasac_bn_tile_stats_reduce only produces `sums` (then all-reduce + dasac_bn_train_finalize = SyncBN). */
int dasac_bn_train_finalize_tiles(const float* tile_stats, int n_tiles, int mpad, double count, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, float momentum, float eps, int C,
                                  float* scale, float* shift, float* mean, float* invstd, dasac_stream_t stream);
int dasac_bn_tile_stats_reduce(const float* tile_stats, int n_tiles, int C, int mpad, double* sums, dasac_stream_t stream);
/* One rank, nothing to all-reduce between statistics and use: finalize + normalise in ONE launch per BN layer
 * (dasac_bn_train_apply_tiles = dasac_bn_train_finalize_tiles + dasac_bn_apply; every block re-adds its channel's tile statistics
 * in the same fixed order), and the whole BN backward in two (dasac_bn_bwd_fused = the reduction's first stage + a dz kernel whose
 * blocks add the (plane, chunk) partials themselves and also write d gamma / d beta; workspace of dasac_bn_stats_workspace bytes). */
int dasac_bn_train_apply_tiles(const float* z, const float* tile_stats, int n_tiles, int mpad, double count,
                               const float* gamma, const float* beta, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, float momentum, float eps, const float* res, int relu,
                               int N, int C, int64_t HW, float* y, float* mean, float* invstd, dasac_stream_t stream);
int dasac_bn_bwd_fused(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma,
                       double count, int N, int C, int64_t HW, float* dz, float* dgamma, float* dbeta,
                       void* workspace, size_t ws_bytes, dasac_stream_t stream);
int dasac_bn_apply(const float* z, const float* scale, const float* shift, const float* res, int relu,
                   int N, int C, int64_t HW, float* y, dasac_stream_t stream);
int dasac_bn_bwd_reduce(const float* dy, const float* z, const float* mean, const float* invstd,
                        int N, int C, int64_t HW, double* sums, float* dgamma /* optional: this rank's sum dy*xhat */,
                        float* dbeta /* optional: this rank's sum dy */, void* workspace, size_t ws_bytes,
                        dasac_stream_t stream);
int dasac_bn_bwd_apply(const float* dy, const float* z, const float* mean, const float* invstd,
                       const float* gamma, const double* sums, double count, const double* count_dev, int N, int C,
                       int64_t HW, float* dz, float* dgamma, float* dbeta, dasac_stream_t stream);

/* Whole-network refresh of the derived operands after an optimiser / EMA step -- what ~100 dasac_bn_fold and ~200
 * dasac_conv_pack calls per step did, in two launches.  `jobs` are DEVICE arrays of the structs below, `chunks` device
 * (job, chunk) int32 pairs: one chunk = 256 channels of a fold job / dasac_pack_chunk_elems() floats of a pack job's output
 * (ceil(Kpad*Mpad / chunk) chunks per job; K and M padding are written as zeros).  Single-branch convolutions only
 * (taps = kh*kw of the one branch); mode / order as in dasac_conv_pack, Mpad = dasac_conv_mpad(M), Kpad = dasac_conv_kpad(K).
 * `jobs` and `chunks` must be 8-byte aligned; the tensors a job points to need element alignment. */
typedef struct dasac_fold_job {
  const float *gamma, *beta, *mean, *var, *conv_bias; /* conv_bias may be NULL */
  float *scale, *shift, *invstd;                      /* all three are written: invstd is NOT optional here */
  float eps;
  int32_t C;
} dasac_fold_job;
typedef struct dasac_pack_job {
  const float* w;     /* [Cout][Cin][taps] */
  const float* scale; /* [Cout] folded into the operand, or NULL */
  float* out;         /* [Kpad/4][Mpad][4] */
  int32_t Cout, Cin, taps, Mpad, Kpad, mode, order, reserved;
} dasac_pack_job;
int dasac_pack_chunk_elems(void);
int dasac_bn_fold_multi(const dasac_fold_job* jobs, const int32_t* chunks, int n_chunks, dasac_stream_t stream);
int dasac_conv_pack_multi(const dasac_pack_job* jobs, const int32_t* chunks, int n_chunks, dasac_stream_t stream);

/* models/sac.py:337-338  `ignore_mask = (y == -1); y[ignore_mask] = 255` in one pass: mask[i] = labels[i] == pad_label,
 * labels[i] = ignore_label there (in place, like the reference).  labels i64 [n], mask u8 [n]. */
int dasac_label_pad_mask(int64_t* labels, uint8_t* mask, int64_t n, int pad_label, int ignore_label,
                         dasac_stream_t stream);
/* nn.Dropout2d(p) in train mode (models/fcn.py:52,56): keep_scale[plane] = Bernoulli(1-p) / (1-p) for the (n, c) planes,
 * consumed by dasac_scale_planes.  Counter-based Philox4x32-10: the draw is a pure function of (seed, offset, plane) --
 * the caller advances `offset` per call; it is NOT ATen's stream (parity tests inject the mask instead).  Plane i draws
 * with counter = (i low word, i high word, offset low word, offset high word) and key = (seed low word, seed high word);
 * u = (first output word >> 8) / 2^24 and the plane is kept iff u >= p.  Requires 0 <= p < 1 and planes > 0. */
int dasac_dropout_planes(uint64_t seed, uint64_t offset, float p, int64_t planes, float* keep_scale,
                         dasac_stream_t stream);

/* Validation counts (utils/metrics.py:9-53, train.py:339-469): counts[0:C] += tp, counts[C:2C] += fp,
 * counts[2C:3C] += fn of argmax_c logits vs gt (pixels with gt == ignore_index skipped); the caller
 * zeroes `counts` (int64 [3*C]) once per evaluation and all-reduces it across ranks. */
int dasac_iou_counts(const float* logits, const int64_t* gt, int B, int C, int64_t HW, int ignore_index,
                     int64_t* counts, dasac_stream_t stream);

/* Validation counts of several mask layers against ONE ground-truth map in one launch (train.py:386-399: one `Jaccard` per
 * layer -- `logits_up`, `teacher_init`, `teacher_refined` through argmax(., 1), `teacher_labels` as it is; utils/metrics.py:18-39
 * `Jaccard.add_sample`).  Up to 4 score tensors fp32 [B,C,HW] (arg-max, first maximum wins) and up to 2 label maps int64
 * [B,HW]; any of the six may be NULL, at least one is not.  The layers are numbered in argument order over the non-NULL
 * pointers, scores first, then label maps.  counts: int64 [L][3][C] = (tp, fp, fn) per layer, ACCUMULATED into (the caller zeroes
 * it once per evaluation and sums it over ranks).  Per pixel: gt == ignore_index is skipped; p == gt adds tp[gt]; otherwise
 * fp[p] if 0 <= p < C and fn[gt] if 0 <= gt < C (a label of 255 over a labelled pixel is a false negative only, gt == -1 a
 * false positive only, as in dasac_iou_counts).  Integer adds only: exact and bit-identical from run to run -- the reference's
 * float32 counters (exact up to 2^24 pixels per class) are not reproduced.  C <= 64.  The ground truth is read once for all
 * layers; no load leaves a buffer (H*W needs no alignment, pointers only that of their element type).  No workspace. */
int dasac_mask_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                      const int64_t* labels0, const int64_t* labels1, const int64_t* gt, int B, int C, int64_t HW,
                      int ignore_index, int64_t* counts, dasac_stream_t stream);

/* Joint tables of the same pass: which class is taken for which, and how often a confidence is right.  The layer slots are those
 * of dasac_mask_counts -- up to 4 score tensors fp32 [B,C,HW] (arg-max, first maximum wins), up to 2 label maps [B,HW], NULL slots
 * skipped, layers numbered over the non-NULL slots, scores first -- but a label map is int64 or, with bit i of `labels_u8_mask`
 * set for slot labels<i>, uint8 at any address (the maps dasac_infer_fuse writes).  gt: int64 [B,HW].
 *   confusion: int64 [L][C+1][C+1], ACCUMULATED into; row = ground truth, column = prediction; a value inside [0, C) is its own
 *     index, every other value (a label map's 255, gt == -1, anything out of range) is index C, "no class".  A pixel with
 *     gt == ignore_index is skipped for every output, and that is checked first.  Hence tp[c] = M[c][c], fp[c] = sum_r M[r][c] -
 *     M[c][c], fn[c] = sum_k M[c][k] - M[c][c] (c < C) are dasac_mask_counts' counts bit for bit, and sum M = the pixels not ignored.
 *   reliability: int64 [Ls][C][n_bins][2] over the Ls score layers, ACCUMULATED into, or NULL (then nothing of it is computed):
 *     [l][p][b][h] with p the arg-max class, h = (p == gt) and b the bin of the winning confidence v -- the winning score itself
 *     when bit l of `softmax_mask` is clear (the layer holds probabilities), 1.0f / sum_c expf(x_c - max_c x) in fp32 when it is set
 *     (the layer holds logits); b = !(v > 0) ? 0 : min(n_bins - 1, (int)(v * n_bins)) with an fp32 multiply: NaN and 0 fall in bin
 *     0, v >= 1 in the last.  1 <= n_bins <= 32.  sum_b [l][p][b][1] = M_l[p][p], sum_b [l][p][b][0] = sum_r M_l[r][p] - M_l[p][p].
 * Integer adds only: exact and bit-identical from run to run.  C <= 64.  No load leaves a tensor; pointers need the alignment of
 * their element type only.  No workspace.  One launch (two when C is close to 64, every slot is used and the tables of all
 * layers exceed one workgroup's LDS). */
int dasac_confusion_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                           const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C,
                           int64_t HW, int ignore_index, int64_t* confusion, int64_t* reliability, int n_bins, int softmax_mask,
                           dasac_stream_t stream);

/* Label-free view consistency: how far the T aligned teacher views of a target image agree -- the signal the method trains on,
 * counted; a diagnostic the reference does not have.  aligned: fp32 [N*T][C][HW], view t of group n at index n*T + t: the tensor
 * dasac_warp_pool writes (`aligned`), probabilities in the reference frame, zero where a view does not reach.  Per group n, pixel p
 * and view t:
 *   z_t      the fp32 sum of the view's C values at the pixel, added one class after another in ascending c: the view's bilinear
 *            coverage there (1 inside, 0 outside, fractional on the rim and next to zeroed padding);
 *   covered  z_t >= cover (0.5: more than half of the tap weight is real);
 *   a_t      the arg-max over c of the view's values, first maximum wins (strict >);
 *   k        the number of covered views;
 *   c*       the consensus: the arg-max over c of sum_t aligned[n,t,c,p], an fp32 sum over ALL t in ascending order, first maximum
 *            wins -- uncovered views add their zeros or rim weights exactly as they do in the pooled sum;
 *   m        the number of covered views with a_t == c*.
 * Three int64 tables, ACCUMULATED into (the caller zeroes them or keeps accumulating):
 *   agree    [C+1][T+1][T+1]: every pixel adds 1 at [c*][k][m] when k >= 1 and at [C][0][0] when k == 0: one call adds N*HW in all;
 *   flips    [C][C]: every pair t < u of views that are both covered adds 1 at [a_t][a_u]; the diagonal holds the agreeing pairs
 *            (the host symmetrises the matrix);
 *   per_view [T][2]: slot t counts the pixels where it is covered, and those where it is covered and a_t == c*.
 * 1 <= T <= DASAC_CONSISTENCY_MAX_VIEWS, 1 <= C <= 32, N > 0, 0 < HW < 2^30 (dasac_warp_pool's own limit) and N*T < 2^31; offsets
 * are 64-bit.  Pointers are non-NULL and aligned to their element size; anything else is DASAC_EINVAL before any launch.  Integer
 * adds only: exact and bit-identical from run to run.  No load leaves its (n, t, c) plane (HW needs no alignment).  One launch on
 * `stream`; no workspace, no allocation, no synchronisation. */
#define DASAC_CONSISTENCY_MAX_VIEWS 8
int dasac_view_consistency(const float* aligned, int N, int T, int C, int64_t HW, float cover, int64_t* agree, int64_t* flips,
                           int64_t* per_view, dasac_stream_t stream);

/* Where in the image the errors are: dasac_mask_counts' counts split by the distance to the nearest class contour -- trimap /
 * boundary-band IoU, interior IoU and Boundary IoU (Cheng et al., 2021) follow from the tables; a diagnostic the reference does not
 * have.  The layer slots are those of dasac_confusion_counts: up to 4 score tensors fp32 [B,C,H,W] (arg-max, first maximum wins), up
 * to 2 label maps [B,H,W], int64 or, with bit i of `labels_u8_mask` set for slot labels<i>, uint8 at any address; NULL slots skipped,
 * layers numbered over the non-NULL slots, scores first.  gt: int64 [B,H,W].
 *   A MAP is one label per pixel (the ground truth, a label map, the arg-max of a score tensor).  Its class index is the value itself
 *   when that lies in [0, C); every other value (255, -1, anything out of range) is "no class".  For a pixel p that holds a class,
 *   d_L(p) is the smallest Chebyshev distance max(|dy|, |dx|) to a pixel q of the SAME image, inside it, that holds a DIFFERENT
 *   class: no-class pixels are transparent (never a contour, never the cause of one), the image border is no contour, the images of
 *   a batch do not see each other.  Equivalently d_L(p) <= r exactly when the class pixels of the (2r+1)^2 window around p are not all
 *   of one class.  slot_L(p) = d_L(p) - 1 when 1 <= d_L(p) <= R, and R otherwise (further than R, no other class in reach, or p holds
 *   no class).
 *   table: int64 [L][R+1][5][C], ACCUMULATED into.  A pixel with gt == ignore_index is skipped for every row, and that is checked
 *   first.  With g the ground truth, a the prediction, sg / sa the pixel's slot in the ground-truth map / in the predicted map:
 *     row 0 tp, 1 fp, 2 fn   exactly dasac_mask_counts' rule (a == g adds tp[g] when g is a class; otherwise fp[a] when a is a
 *                            class and fn[g] when g is a class), at slot sg;
 *     row 3 pred             +1 at class a when a is a class, at slot sa;
 *     row 4 both             +1 at class a when a == g is a class, at slot max(sg, sa).
 *   The predicted map's distances are taken over the whole map, ignored pixels included as neighbours; only the counting skips
 *   them.  Summed over the slots the rows are dasac_mask_counts' tp, fp, fn, tp + fp and tp bit for bit; the band of width r is the
 *   slots < r, the interior the slots >= r, and Boundary IoU of class c at radius r is I / (G + P - I) with G = sum (tp + fn),
 *   P = sum pred, I = sum both over the slots < r.
 * 1 <= R <= DASAC_BOUNDARY_MAX_RADIUS, 1 <= C <= 64, B, H, W >= 1 with any alignment; offsets are 64-bit.  gt, table and the
 * workspace are non-NULL, at least one layer is; fp32 / int64 tensors are aligned to their element size, the workspace to 16
 * bytes and holds dasac_boundary_counts_workspace(layers, B, H, W) bytes (`layers` = the non-NULL slots; one uint8 map each and one
 * for the ground truth -- an upper bound, since a uint8 label map is staged from where it is and the call asks for no map for it).
 * Anything else is DASAC_EINVAL before any launch.  Integer adds only: exact, bit-identical from run to run and independent of tile order.  The
 * scores are read once (arg-maxed into uint8 maps in the workspace, which the stencil then stages tile by tile with an R-wide
 * halo); no load leaves a tensor.  Two launches on `stream`; no allocation, no synchronisation. */
#define DASAC_BOUNDARY_MAX_RADIUS 16
size_t dasac_boundary_counts_workspace(int layers, int B, int H, int W);
int dasac_boundary_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                          const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C, int H,
                          int W, int R, int ignore_index, int64_t* table, void* workspace, size_t ws_bytes, dasac_stream_t stream);

/* On which OBJECTS the errors are: connected-component labelling of a label map, the size-stratified segment tables built on it and
 * the removal of specks; a diagnostic the reference does not have.
 *   A MAP is one label per pixel.  Its class is the value itself when that lies in [0, C); every other value (255, -1, anything out
 *   of range) is "no class".  Two pixels of one image are ADJACENT under connectivity 4 when they share an edge, under connectivity 8
 *   when they share an edge or a corner.  A SEGMENT is a maximal set of pixels of the same class connected through adjacent pixels
 *   of that class; no-class pixels belong to no segment.  The images of a batch do not see each other, and a run that ends at the
 *   right edge of row y is not adjacent to one that starts at the left edge of row y + 1.  A segment's ROOT is the smallest y*W + x
 *   among its pixels, its SIZE its pixel count, its BIN min(floor(log2(size)), DASAC_SEGMENT_BINS - 1).
 *
 * dasac_label_segments: labels int64 [B,H,W], or uint8 at any address when `labels_u8` is set.  segment: int32 [B,H,W], the root of
 * the pixel's segment, -1 for a no-class pixel; size: int32 [B,H,W], the size of the pixel's segment, 0 for a no-class pixel; may be
 * NULL.  1 <= C <= 255, connectivity 4 or 8, B, H, W >= 1, H*W <= 2^31 - 1; batch offsets are 64-bit.  Roots are canonical by
 * definition, so the result is a function of the input alone: bit-identical from run to run whatever the block order.  It asks
 * for no workspace (the parents are built in `segment`, the counts in `size`); at most four launches.
 *
 * dasac_segment_counts: the layer slots of dasac_boundary_counts (up to 4 fp32 score tensors, arg-max with the first maximum
 * winning; up to 2 label maps, int64 or uint8 by `labels_u8_mask`; NULL slots skipped, layers numbered over the non-NULL slots,
 * scores first); gt int64 [B,H,W]; 1 <= C <= 64.  table: int64 [L][2][DASAC_SEGMENT_BINS][4][C], ACCUMULATED into.  A ground-truth
 * pixel equal to ignore_index is no-class in the ground-truth map, and that is checked first.  With g the ground truth and a the
 * layer's prediction:
 *   side 0, ground-truth segments (computed once per call, shared by all layers): for each segment S of class c, size s, bin b, with
 *     m = #{p in S : a(p) == c}, at [layer][0][b][.][c]: row 0 += 1, row 1 += s, row 2 += m, row 3 += 1 when 2*m > s (the object
 *     was found);
 *   side 1, predicted segments, taken over the whole predicted map, ignored pixels included as members and neighbours: for each
 *     segment S of class c, size s, bin b (binned by s), with n = #{p in S : g(p) != ignore_index} and m = #{p in S : g(p) == c
 *     and not ignored}: a segment with n == 0 is counted nowhere; otherwise row 0 += 1, row 1 += n, row 2 += m, row 3 += 1 when
 *     2*m > n (the segment is real, not a speck).
 *   Summed over the bins these hold bit for bit against dasac_mask_counts: side 0 row 2 = tp, side 0 row 1 = tp + fn,
 *   side 1 row 1 = tp + fp, side 1 row 2 = tp.
 * The workspace holds dasac_segment_counts_workspace(layers, B, H, W) bytes (`layers` = the non-NULL slots) and is aligned to 16
 * bytes; 4 + 4 L launches (one fewer per map when an image is a single tile: nothing to merge).
 *
 * dasac_segment_filter: `out` has the dtype and shape of `labels`; a pixel whose segment has size < min_size gets `fill` (which must
 * fit the dtype), every other pixel, no-class pixels included, keeps its value; min_size <= 1 copies the map.  `out` may NOT
 * alias or overlap `labels`: DASAC_EINVAL.  1 <= C <= 255.
 *
 * For all three: fp32 / int64 / int32 tensors are aligned to their element size; anything else is DASAC_EINVAL before any launch.
 * Integer arithmetic only, exact and bit-identical from run to run; no load or store leaves a tensor or the workspace at any
 * alignment of a uint8 map; no allocation, no synchronisation, and no kernel waits for another workgroup. */
#define DASAC_SEGMENT_BINS 24
size_t dasac_label_segments_workspace(int B, int H, int W);
int dasac_label_segments(const void* labels, int labels_u8, int B, int C, int H, int W, int connectivity, int32_t* segment,
                         int32_t* size, void* workspace, size_t ws_bytes, dasac_stream_t stream);
size_t dasac_segment_counts_workspace(int layers, int B, int H, int W);
int dasac_segment_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                         const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C, int H,
                         int W, int connectivity, int ignore_index, int64_t* table, void* workspace, size_t ws_bytes,
                         dasac_stream_t stream);
size_t dasac_segment_filter_workspace(int B, int H, int W);
int dasac_segment_filter(const void* labels, int labels_u8, int B, int C, int H, int W, int connectivity, int min_size, int fill,
                         void* out, void* workspace, size_t ws_bytes, dasac_stream_t stream);

/* Mean-field refinement of an inference label map: a locally connected CRF (the ConvCRF form of Teichmann & Cipolla, 2018: truncated
 * Gaussian kernels on a dilated window, Potts compatibility) over the fused class probabilities and the image -- the step DeepLabv2's
 * published pipeline ends in; the reference only kept a place for it (infer_val.py:134).
 *   probs P: fp32 [B,C,H,W], class probabilities as dasac_infer_fuse writes them; image I: fp32 [B,Ci,H,W], the image as the network
 *   sees it (normalised): theta_beta is in the image's own units.
 *   unary and start   u_i[c] = log(max(P_i[c], 1e-20)); Q^0 = P as given, not renormalised.
 *   taps              offsets o = (d a, d b) for a, b in [-r, r], (a, b) != (0, 0), in row-major order of (a, b); a neighbour
 *                     j = i + o counts only when it lies inside the image.
 *   kernel weight     k_ij = w_app exp(-|o|^2 / (2 theta_alpha^2) - sum_ch (I_i - I_j)^2 / (2 theta_beta^2))
 *                            + w_smooth exp(-|o|^2 / (2 theta_gamma^2)), |o| in pixels.
 *   message           den_i = sum_j k_ij; m_i[c] = sum_j k_ij Q^(t-1)_j[c] / den_i when den_i > 0, else 0: a convex combination, so
 *                     border pixels and 1 x 1 images need no special case.
 *   update            Q^t_i = softmax_c(u_i[c] + compat m_i[c]), all pixels in parallel from Q^(t-1).
 *   after n_iter updates: labels uint8 [B,H,W] = lut[argmax_c Q] (lut: uint8, at least C entries) or the arg-max itself when lut is
 *   NULL, first maximum wins; conf (optional) fp32 [B,H,W], the winning Q; probs_out (optional) fp32 [B,C,H,W], Q itself.
 * 1 <= C <= 32, 1 <= Ci <= 4, 1 <= r <= 5, 1 <= d <= 4 with r d <= 8, 1 <= n_iter <= 16; the thetas > 0; w_app, w_smooth >= 0 with a
 * positive sum; compat >= 0, all finite; B, H, W >= 1, any H and W; every tensor below 4 GiB - 4 KiB.  probs, image and labels are
 * non-NULL, fp32 pointers aligned to 4 bytes and nothing more; outputs and workspace overlap neither the inputs nor each other.  The
 * workspace is aligned to 16 bytes and holds dasac_crf_meanfield_workspace(B, C, H, W, n_iter) bytes: the Q buffers the iterations
 * alternate between (one for n_iter == 1, else two); less is DASAC_EWORKSPACE, anything else above DASAC_EINVAL, both before any
 * launch.  One launch per iteration on `stream`, the last one fusing arg-max, LUT and confidence; the taps are summed in their order
 * by one thread per pixel, no atomics: the same bits on every run and wherever the tensors lie.  No load or store leaves a tensor;
 * no allocation, no synchronisation. */
size_t dasac_crf_meanfield_workspace(int B, int C, int H, int W, int n_iter);
int dasac_crf_meanfield(const float* probs, const float* image, int B, int C, int Ci, int H, int W, int radius, int dilation,
                        float w_app, float theta_alpha, float theta_beta, float w_smooth, float theta_gamma, float compat, int n_iter,
                        const uint8_t* lut, uint8_t* labels, float* conf, float* probs_out, void* workspace, size_t ws_bytes,
                        dasac_stream_t stream);

/* Per-image class statistics for importance-sampled target selection (tools/compute_IS_weights.py:58-83, on the device):
 * counts[b][v] += number of pixels of image b with value v, v in 0..255 (value 255 is counted too; callers drop it).
 * labels: [B][HW] uint8, any alignment (an unaligned head and a tail of any length per image are read byte by byte, the
 * rest 16 bytes per lane; no load leaves [labels, labels + B*HW)).  counts: [B][256] int64, accumulated into (the caller
 * zeroes it).  Integer adds only: exact, and bit-identical from run to run.  No workspace. */
int dasac_label_hist(const uint8_t* labels, int B, int64_t HW, int64_t* counts, dasac_stream_t stream);

/* K augmented views of one target crop: the pixel work of DataTarget.__getitem__'s tail
 * (datasets/dataloader_target.py:281-306) -- GuidedRandHFlip (datasets/tf_target.py:141-157), MaskRandScaleCrop
 * (:159-239; Pillow resize BILINEAR for the image, NEAREST for label / padding mask) and ToTensorMask / Normalize /
 * ApplyMask (:33-98) -- for all L views in one launch, byte-exact with Pillow's fixed-point resampling.
 * image u8 [3,H,W] planar, label u8 [H,W], mask u8 [H,W] or NULL (0 = valid); `tables`: L rows of
 * dasac_make_views_table_ints(H, W) int32 built on the host (views.py: view_tables): header {flip, ii, jj, win_h,
 * win_w, identity, 0, 0}, bounds_h[W][2], coeff_h[W][8], bounds_v[H][2], coeff_v[H][8], nearest_x[W], nearest_y[H].
 * mean3 / std3: HOST arrays of 3 floats.  Outputs: frames f32 [L,3,H,W] (normalised, 0 under the mask), gt i64
 * [L,H,W] (ignore_label under the mask), views_u8 (optional) u8 [L,3,H,W] = the resampled bytes. */
int dasac_make_views_table_ints(int H, int W);
int dasac_make_views(const uint8_t* image, const uint8_t* label, const uint8_t* mask, int H, int W, int L,
                     const int32_t* tables, const float* mean3, const float* std3, int ignore_label, float* frames,
                     int64_t* gt, uint8_t* views_u8, dasac_stream_t stream);

/* Photometric augmentations of the student's views (second half): `tf_augm` of DataTarget
 * (datasets/dataloader_target.py:116-123,292-296) = RandGaussianBlur (datasets/tf_target.py:331-349), MaskRandJitter
 * (:365-390, torchvision ColorJitter) and MaskRandGreyscale (:351-363) on the u8 views dasac_make_views emits, then
 * ToTensorMask / Normalize / ApplyMask (:33-98) -> frames1.  Byte-exact with Pillow's BoxBlur.c / Blend.c / Convert.c.
 * views_u8 u8 [L,3,H,W] (L <= 16); gt i64 [L,H,W] from dasac_make_views or NULL (pixels with gt == ignore_label are
 * the padding: frame value 0).  `params`: HOST array of L rows of DASAC_PHOTO_PARAMS doubles:
 *   [0] Gaussian radius (<= 0: no blur)        [1] colour jitter on/off
 *   [2..5] order of the four adjustments (0 brightness, 1 contrast, 2 saturation, 3 hue)
 *   [6..9] brightness, contrast, saturation, hue factors        [10] greyscale on/off        [11] reserved
 * Outputs: frames f32 [L,3,H,W]; out_u8 (optional) the augmented bytes.  `workspace`: device scratch of
 * dasac_view_photometric_workspace(H, W, L) bytes. */
#define DASAC_PHOTO_PARAMS 12
size_t dasac_view_photometric_workspace(int H, int W, int L);
int dasac_view_photometric(const uint8_t* views_u8, const int64_t* gt, int H, int W, int L, const double* params,
                           const float* mean3, const float* std3, int ignore_label, float* frames, uint8_t* out_u8,
                           void* workspace, size_t ws_bytes, dasac_stream_t stream);

/* Source crops and the target front half (the host work in front of dasac_make_views): the source loader DLSeg
 * (datasets/dataloader_seg.py:70-113,141-161: MaskRandScale tf_seg.py:129-153, MaskRandHFlip :202-211, MaskRandCrop with
 * pad_if_needed :155-187, MaskCenterCrop / MaskScale for eval, the "game" pre-resize) and DataTarget.tf_pre
 * (datasets/dataloader_target.py:101-107: MaskScale tf_target.py:127-139, MaskRandScale :241-263, MaskRandCrop :265-303,
 * MaskRandHFlip :318-329), byte-exact with Pillow's resize (BILINEAR image, NEAREST label), then ToTensorMask / Normalize /
 * ApplyMask.  B images per launch, each of its own size, packed back to back:
 *   images  u8, image b at desc[b][0]: HWC-interleaved as decoded (pixel stride 3, channel stride 1) or planar (1, H*W);
 *   labels  u8 [H,W] at desc[b][1];  `images_bytes` / `labels_bytes` = the buffers' sizes;
 *   desc    DEVICE int64 [B][DASAC_CROP_DESC]: {image offset, label offset, H, W, pixel stride, channel stride, scaled H,
 *           scaled W, table offset (int32 elements into `tables`; -1 = identity, scaled size = source size), flip (0 none,
 *           1 mirror the scaled image = flip before the crop, 2 mirror the crop = flip after it), pad_t, pad_l, crop i,
 *           crop j, output image offset, output label offset (the last two: dasac_resize_u8 only)};
 *   tables  DEVICE int32, per scaled image dasac_crop_table_ints(SH, SW) ints laid out as the body of a dasac_make_views row:
 *           bounds_h[SW][2], coeff_h[SW][8], bounds_v[SH][2], coeff_v[SH][8], nearest_x[SW], nearest_y[SH] (an unchanged axis
 *           gets identity tables: one Pillow pass); `table_ints` = the buffer's length.
 * Descriptors are range-checked on the device against the buffer sizes: an image whose regions do not fit is skipped by
 * dasac_resize_u8 and reads as padding in dasac_make_crops.
 * dasac_resize_u8   the whole scaled image of every descriptor: planar u8 [3,SH,SW] at out_images + desc[b][14], u8 label
 *                   [SH,SW] at out_labels + desc[b][15].  max_pixels = the largest SH*SW (sizes the grid).
 * dasac_make_crops  the Hc x Wc crop of every descriptor's scaled image in one launch: crop window (i, j) of the image padded by
 *                   (pad_t, pad_l) (image / label 0, mask 1 in the padding), flip, then mean3 / std3 (HOST, 3 floats each).
 *                   Outputs, each optional: frames f32 [B,3,Hc,Wc] (0 in the padding), labels_out i64 [B,Hc,Wc] (ignore_label
 *                   in the padding), image_u8 u8 [B,3,Hc,Wc], label_u8 u8 [B,Hc,Wc], mask_u8 u8 [B,Hc,Wc] (1 = padding):
 *                   the last three are what dasac_make_views takes. */
#define DASAC_CROP_DESC 16
int dasac_crop_table_ints(int SH, int SW);
int dasac_resize_u8(const uint8_t* images, int64_t images_bytes, const uint8_t* labels, int64_t labels_bytes, int B,
                    const int64_t* desc, const int32_t* tables, int64_t table_ints, int max_pixels, uint8_t* out_images,
                    int64_t out_images_bytes, uint8_t* out_labels, int64_t out_labels_bytes, dasac_stream_t stream);
int dasac_make_crops(const uint8_t* images, int64_t images_bytes, const uint8_t* labels, int64_t labels_bytes, int B,
                     const int64_t* desc, const int32_t* tables, int64_t table_ints, int Hc, int Wc, const float* mean3,
                     const float* std3, int ignore_label, float* frames, int64_t* labels_out, uint8_t* image_u8,
                     uint8_t* label_u8, uint8_t* mask_u8, dasac_stream_t stream);

/* The trainer's epoch summary panels (base_trainer.py:75-198 `BaseTrainer._visualise`; helpers `_apply_cmap` :228-248,
 * `_error_rgb` :250-256, `_visualise_grid` :258-270), rendered on the device: ONE launch renders every panel of every image of
 * a batch into the strip float32 [B,3,h,P*w] (the reference's `visuals`, panel p in columns [p*w, (p+1)*w)) and, when rows_u8
 * is not NULL, into u8 [B,3,h,P*w] = trunc(clamp(255 * strip, 0, 255)) (:264).  `jobs`: DEVICE array of n_jobs records,
 * `jobs_host` the same records on the HOST (the arguments are checked on it).  Per job, by `kind`:
 *   DASAC_VIS_IMAGE   src f32 [B,3,H,W]: downsize(src * std + mean)                                             (:119,:148,:172)
 *   DASAC_VIS_LABELS  src i64 [B,H,W]: values saturated to 0..255 -> palette at the four taps -> / 255 -> downsize (:123-131)
 *   DASAC_VIS_SCORES  src f32 [B,C,H,W]: softmax over C at each tap when `softmax`, every class resized, max / FIRST arg-max;
 *                     the class colours go to `column`, inferno(1 - max) to `column2`                      (:134-145,:152-165)
 *   DASAC_VIS_CONF    src f32 [B,H,W]: inferno(1 - downsize(src))                                                 (:179-183)
 * downsize = bilinear, align_corners=True (:99-109), shrinking or enlarging, any H x W, output extent 1 included.  Every kind
 * but IMAGE is blended: 0.3 * downsize(backdrop * std + mean) + 0.7 * colours, backdrop f32 [B,3,H,W] of the job's H x W.
 * palette: DEVICE u8 [256][3]; cmap: DEVICE f32 [256][3], indexed by trunc(256 * v) clipped to 0..255; mean3 / std3: HOST
 * arrays of 3 floats.  Every tap index is clamped inside its plane: no load leaves a tensor of the stated shape.
 * dasac_vis_grid: torchvision's make_grid(nrow=1, padding, pad_value) of the quantised rows (:269): for B > 1 u8
 * [3][B*(h+padding)+padding][wt+padding] filled with trunc(255 * pad_value), row k at y = k*(h+padding)+padding, x = padding;
 * for B == 1 the row itself, [3][h][wt].  strip f32 [B,3,h,wt]. */
#define DASAC_VIS_IMAGE 0
#define DASAC_VIS_LABELS 1
#define DASAC_VIS_SCORES 2
#define DASAC_VIS_CONF 3
typedef struct dasac_vis_job {
  const void* src;
  const float* backdrop; /* NULL for DASAC_VIS_IMAGE */
  int32_t kind, C, H, W, softmax, column, column2, reserved;
} dasac_vis_job;
int dasac_vis_panels(const dasac_vis_job* jobs, const dasac_vis_job* jobs_host, int n_jobs, int B, int h, int w, int P,
                     const float* mean3, const float* std3, const uint8_t* palette, const float* cmap, float* strip,
                     uint8_t* rows_u8, dasac_stream_t stream);
int dasac_vis_grid(const float* strip, int B, int h, int wt, int padding, float pad_value, uint8_t* grid,
                   dasac_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DASAC_HIP_H */
