/*
 * radmmm_hip.h -- C ABI of libradmmm_hip.so: hand-written gfx950 (MI355X) kernels for
 * the RAD-MMM flow-decoder training step.
 *
 * The reference (NVIDIA/RAD-MMM) is pure Python/PyTorch and has NO C/FFI boundary
 * (SURVEY.md §8b): its plug-in mechanism is jsonargparse `class_path`
 * (configs/RADTTS_model_config.yaml:16-48, tts_main.py:64-65).  The drop-in is
 * therefore the Python package `rad_mmm_amd` (same ctor kwargs / forward signature /
 * state_dict names as decoders.RADMMMFlow and loss.RADMMMLoss); THIS header is the
 * boundary underneath it, i.e. what a binding for the reference's operators would
 * bind.  Each entry point cites the reference code whose arithmetic it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; radmmm_last_error() returns a
 *    thread-local message for the last failure on the calling thread.
 *  - all pointers are DEVICE pointers into caller-owned memory (no ownership
 *    transfer, no allocation inside the library, no internal threads, no global
 *    mutable state apart from the error string).
 *  - every call takes the hipStream_t to launch on (as void*) and is asynchronous.
 *  - activations are CHANNELS-LAST fp32: a [B, C, T] tensor of the reference is held
 *    as a row-major matrix [B*T rows][ld floats] with row r = b*T + t.  ld % 4 == 0
 *    and 16-byte aligned bases are required wherever a matrix feeds a GEMM.
 *  - `lens` is an int32 device array [B] of valid frames per item (already divided by
 *    n_group_size); NULL means all T frames valid.
 */
#ifndef RADMMM_HIP_H
#define RADMMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RADMMM_ABI_VERSION 4

typedef void* radmmm_stream_t; /* hipStream_t */

const char* radmmm_last_error(void);
int radmmm_abi_version(void);

/* activation codes (forward) / derivative-from-output codes (backward) */
enum { RADMMM_ACT_NONE = 0, RADMMM_ACT_SOFTPLUS = 1, RADMMM_ACT_RELU = 2, RADMMM_ACT_LEAKY = 3 };
/* scaling functions of the affine coupling, common.py:1127-1140 */
enum { RADMMM_SCALE_TANH = 0, RADMMM_SCALE_EXP = 1, RADMMM_SCALE_SIGMOID = 2, RADMMM_SCALE_TRANSLATE = 3 };

/* ------------------------------------------------------------------------------------
 * Split formats of the row-major operand copies (one K-contiguous row per frame / output channel):
 *   RADMMM_SPLIT_F16  two half arrays [rows][ld]: hi = fp16(t), lo = fp16(t - hi), t = scale * x clamped to +-60000
 *   RADMMM_SPLIT_X8A  hi as above + the 8-bit CROSS array in place of lo, same row pitch (2*ld bytes), ld % 32 == 0:
 *                     per 32 columns 64 bytes [ e4m3(t * 2^e) x 32 | e4m3((t - hi) * 2^(11+e)) x 32 ]  (A role)
 *   RADMMM_SPLIT_X8B  the same with the two 32-byte halves swapped [ lo8 | hi8 ]                     (B role, weights)
 * e4m3 = OCP FP8 E4M3, round to nearest even, saturated at +-448.  A block-scaled FP8 MFMA of an X8A fragment with an
 * X8B fragment yields Ah.Bl + Al.Bh (radmmm_rowgemm_h3 with nprod = 2).
 * Non-finite inputs: +-Inf is clamped like any large value (+-60000, flag bit 0, and bit 1 with level 6 in an 8-bit format).
 * NaN is NOT propagated and NOT reported: the clamp (v_med3_f32) turns it into -60000, so every store path -- the 4-wide and
 * the 1-wide store of csrc/split_pack.h and the GEMM epilogues' pair store -- writes hi = 0xfb53 (-60000), lo = 0,
 * hi8 = 0xfe (-448), lo8 = 0, and raises no flag bit (the flag's amax ignores NaN, as fmaxf does).  A caller that must see
 * a NaN again passes it on by other means (radmmm_weightnorm_bwd's `poison`).  tests/_split_ref.py is the host model of
 * these formats; tests/test_hip_split_direct.py holds the producers to it bit for bit.
 * ------------------------------------------------------------------------------------ */
#define RADMMM_SPLIT_F16 0
#define RADMMM_SPLIT_X8A 1
#define RADMMM_SPLIT_X8B 2
/* options of a split producer: format, exponent e of the 8-bit parts, optional saturation flag (device int, OR-ed with
 * bit 0 when |scale * x| > 60000 was clamped; with bit 1 when an element's 8-bit parts left e4m3's range (|scale * x| *
 * 2^e > 448: that element keeps single-product accuracy) and then also, one-hot, with bit 1 + L, L = ceil(log2(|scale * x|
 * * 2^e / 448)) clamped to 1 .. 6: by how many powers of two e was too large) */
typedef struct { int fmt; int x8_exp; int32_t* sat_flag;
                 void* lo16; /* optional, 8-bit formats only: the fp16 lo part fp16(s*x - hi) as well, same pitch as the hi
                                array (radmmm_wn_input_fwd, radmmm_dact_mul_transposed): feeds radmmm_wgrad_rm */
} radmmm_split_opts;

/* ------------------------------------------------------------------------------------
 * Row GEMM with taps: the Conv1d family in channels-last form, fp32 MFMA
 * (v_mfma_f32_32x32x2_f32, exact fp32).
 *
 *   acc[r, n] = sum_{tap} sum_{k<K} Am[r + shift(tap), k] * Bt[tap](k, n)
 *   shift(tap) = sign * (tap - taps/2) * dil
 *   Am[row, :] = A[row, :] if the shifted frame lies in the same item and inside
 *                [0, T) (a_mask_mode 0) or [0, lens[b]) (a_mask_mode 1), else 0
 *   Bt[tap](k, n) = B[tap*b_tap_stride + n*ldb + k]   (b_layout 0: [N][K], forward)
 *                 = B[tap*b_tap_stride + k*ldb + n]   (b_layout 1: [K][N], data-grad)
 *
 * Epilogue, applied in this order to v = acc:
 *   pconv     : v *= taps_r / (cnt + 1e-6), cnt = #taps of a (ratio_taps, ratio_dil)
 *               window centred on r whose frame is < lens[b]  (0 if cnt == 0)
 *   premask   : v *= [t < lens[b]]
 *   bias      : v += bias[n]
 *   add       : v += add[r*ldadd + n]
 *   postmask  : v *= [t < lens[b]]
 *   dact      : v *= act'(y) expressed from the saved OUTPUT y = dact_src[r*lddact+n]
 *               (softplus: 1 - exp(-y); relu: y > 0; leaky: y > 0 ? 1 : 0.01)
 *   rowscale  : 1: v *= mask ; 2: v *= mask * ratio (same ratio definition as pconv)
 *   act       : v = act(v)
 *   C[r*ldc+n] = v ;  if C2: C2[r*ldc2+n] = (c2_accum ? C2[...] : 0) + v
 *
 * Replaces: F.conv1d / PartialConv1d / ConvNorm / weight-normed 1x1 convs and their
 * autograd data-gradients (common.py:179-191, 816-835; partialconv1d.py:58-94), and
 * the invertible 1x1 channel mix (common.py:546, 615).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  const float* A; int lda;
  int64_t a_item_stride; /* 0: row r at A + r*lda; else item b, frame t at A + b*a_item_stride + t*lda
                            (rows of one item may then overlap: lda < K is allowed, STFT framing).  With a_mask_mode 1
                            an item may hold more frames than the T that are written (lens[b] > T, the inverse STFT's
                            F = T + 1): a tap then reads frames up to min(lens[b], T + taps/2 * dil) - 1 of that item,
                            the last item included, so the caller's buffer must hold every frame below lens[b] */
  const float* B; int ldb; int64_t b_tap_stride; int b_layout;
  float* C; int ldc;      /* radmmm_rowgemm_h3: may be NULL when Ch is given (no fp32 copy of the result is written) */
  int M, N, K;
  int taps, dil, sign;
  int T;                 /* frames per item; M must be a multiple of T */
  const int32_t* lens;   /* [M/T] or NULL */
  int a_mask_mode;
  const float* bias;
  int pconv, premask, postmask;
  int ratio_taps, ratio_dil;
  const float* add; int ldadd;
  const float* dact_src; int lddact; int dact;
  int rowscale;
  int act;
  float* C2; int ldc2; int c2_accum;
  /* optional split-fp16 copies of the outputs (operands of the next split-f16 GEMM):
   * Ch/Cl [M][ldch] halves receive hi/lo of ch_scale * C, C2h/C2l of c2h_scale * C2 (ld % 4 == 0) */
  void* Ch; void* Cl; int ldch; float ch_scale;
  void* C2h; void* C2l; int ldc2h; float c2h_scale;
  /* split format of Ch/Cl and C2h/C2l (RADMMM_SPLIT_*, see "split formats" below) and the exponents of their 8-bit parts */
  int split_fmt; int ch_x8_exp; int c2h_x8_exp;
  int32_t* sat_flag;     /* optional device int: saturation report of the split outputs, bits as in radmmm_split_opts.sat_flag */
  void* Clo;             /* optional, with Ch and an 8-bit split_fmt: [M][ldch] halves, the fp16 lo part fp16(ch_scale*v - Ch)
                            as well (the row-major pair Ch / Clo is what radmmm_wgrad_rm contracts) */
  /* optional (radmmm_rowgemm_h3 only): colsum_out[n] = sum over the rows r inside their utterance's length (all rows when
   * the launch has no row scale) of the epilogue's value BEFORE its row scale -- x_r[n] of step (6) below, after the
   * act' factor.  With rowscale = 2 this is the bias gradient of the partial conv whose data gradient the launch computes
   * (common.py:179-191 backward), i.e. radmmm_colsum(C, row_weight 2) without the pass over C: the kernels with the direct
   * epilogue sum it from the accumulators (one partial row per row tile in colsum_scratch, added up in a fixed order:
   * deterministic), every other path runs radmmm_colsum on C afterwards.  colsum_scratch: device scratch of
   * radmmm_rowgemm_h3_colsum_scratch_floats(M, N) floats. */
  float* colsum_out; float* colsum_scratch;
  /* optional (radmmm_rowgemm_h3; ABI 3): the dact step reads the saved OUTPUT y from its row-major 8-bit split copy instead
   * of an fp32 array -- dact_h [M][lddact_h] fp16 hi, dact_x the RADMMM_SPLIT_X8A cross array of the same tensor, both
   * written with scale 1 and exponent dact_x8_exp:  y = hi + e4m3_lo * 2^-(11 + dact_x8_exp)   (within 2^-15 |y| of the
   * fp32 value the pair was split from; the softplus derivative 1 - exp(-y) then carries <= 1.2e-5 absolute).  dact_src
   * must be NULL then.  With it a producer need not keep an fp32 copy of an activation beside its split pair:
   * radmmm_rowgemm_h3 accepts C == NULL when Ch is given (the split copy alone carries the result). */
  const void* dact_h; const void* dact_x; int lddact_h; int dact_x8_exp;
  /* optional (ABI 4): the value that goes to C2 / C2h is  ((c2_src[0] + c2_src[1]) + c2_src[2]) + y  instead of C2 + y --
   * n_c2_src = 1 .. 3 fp32 arrays [M][ldc2] (0: the read-modify-write of C2 as before; c2_accum is ignored otherwise).  The
   * LAST res/skip layer of a WN adds the earlier layers' outputs itself (same association as the running sum, so the same
   * bits), and the earlier layers write their own output only: the skip sum is neither read nor written four times.  C2
   * may then be NULL when C2h is given (only the split copy of the sum is kept). */
  const float* c2_src[3]; int n_c2_src;
} radmmm_rowgemm_desc;

int radmmm_rowgemm_f32(const radmmm_rowgemm_desc* d, radmmm_stream_t stream);

/* Same operation on the f16 matrix cores with fp32-class accuracy by operand splitting
 * (x*s = hi + lo in fp16;  A.B ~= Ah.Bh + Ah.Bl + Al.Bh, fp32 accumulate; measured 2.2e-6 max
 * rel. error at K=5120 vs 3.8e-6 for the fp32 MFMA, at 2.3x its rate).  d->A / d->B are ignored;
 * the operands are the split copies below, both K-CONTIGUOUS:
 *   Ah/Al [M][lda_h] halves (rows = frames, same shift/masking rules as radmmm_rowgemm_f32)
 *   Bh/Bl [taps][N][ldb_h] halves (tap stride b_tap_stride_h halves); b_layout must be 0 --
 *   the data-gradient uses a transposed split copy of the weights instead of layout 1.
 * acc is multiplied by acc_scale (= 1/(a_scale*b_scale)) before the epilogue.
 * Requires K % 32 == 0, lda_h/ldb_h % 8 == 0. */
typedef struct {
  radmmm_rowgemm_desc base;
  const void* Ah; const void* Al; int lda_h;
  const void* Bh; const void* Bl; int ldb_h; int64_t b_tap_stride_h;
  float acc_scale;
  int nprod;                  /* 0 or 3: split products Ah.Bh + Ah.Bl + Al.Bh (fp32-class accuracy);
                                 1: Ah.Bh only = plain fp16 operands, fp32 accumulate (16-bit throughput mode);
                                 2: Ah.Bh on the f16 pipe + both cross terms in ONE block-scaled FP8 MFMA per 32-deep k
                                    step: Al / Bl are then the 8-bit cross arrays RADMMM_SPLIT_X8A / RADMMM_SPLIT_X8B */
  int a8_exp, b8_exp;         /* nprod 2: exponents e the 8-bit parts of A / B were written with (values * 2^e) */
  /* optional EXTRA K segment after the taps: one more "tap" with shift 0 whose A rows start extra_a_rows rows below row 0
   * of Ah/Al (a second activation matrix stored behind the first in the same allocation, same lda_h) and whose weights
   * are tap index `taps` of Bh/Bl: acc += A2 . B[taps].  Sums two GEMMs that share their output (the data gradient of a
   * k-tap conv and of a 1x1 conv reaching the same tensor) in one launch, without the intermediate tensor. */
  int extra_tap; int extra_a_rows;
} radmmm_rowgemm_h3_desc;

int radmmm_rowgemm_h3(const radmmm_rowgemm_h3_desc* d, radmmm_stream_t stream);
int64_t radmmm_rowgemm_h3_colsum_scratch_floats(int M, int N);
/* Additive entry point of ABI 4, read-only: which kernel the calling thread's last radmmm_rowgemm_h3 launch took, as
 * RADMMM_H3_KERNEL_CODE(family, products, mb, epilogue kind); 0 = no launch yet on this thread.  family: the 128 x 128
 * kernel (NARROW; mb reads 4, the kind 0), the per-tap wide kernel rowgemm_h3d, the shared-window kernel rowgemm_win or
 * the one-tap kernel rowgemm_one.  products: 1, 2 or 3 (nprod 0 reads as 3).  mb: tile height / 32 (4 .. 8).  kind: 0 the
 * generic LDS-parking epilogue, 1 PLAIN (C), 2 SPLIT (C + Ch / Cl), 3 RES (C + C2), 4 DGRAD (C + split copy, times act').
 * It is recorded from the launch decision, for every family before the first HIP call (one thread-local store on the host
 * per launch), so also when the launch itself then fails; a refused descriptor leaves it alone.  Tests use it to make sure
 * a shape reached the kernel they mean to test. */
#define RADMMM_H3_FAMILY_NARROW 1
#define RADMMM_H3_FAMILY_H3D 2
#define RADMMM_H3_FAMILY_WIN 3
#define RADMMM_H3_FAMILY_ONE 4
#define RADMMM_H3_KERNEL_CODE(family, nprod, mb, ek) ((family) * 1000 + (nprod) * 100 + (mb) * 10 + (ek))
int radmmm_rowgemm_h3_last_kernel(void);
/* Additive entry point of ABI 4, host only: which kernel radmmm_rowgemm_h3 would launch for a descriptor, as the same
 * RADMMM_H3_KERNEL_CODE; < 0: the descriptor would be refused (same code and radmmm_last_error text as the entry point: both
 * take the decision from one function, and so does radmmm_rowgemm_h3_colsum_rows).  It dereferences no operand pointer (the
 * pointers' presence and alignment is all it looks at) and its only HIP call is the once-per-process CU count behind
 * radmmm_gemm_cu_slots, which reads 256 without a device: it answers on a machine without a GPU, with the MI355X's tile
 * heights.  After a launch, radmmm_rowgemm_h3_last_kernel equals it. */
int radmmm_rowgemm_h3_plan(const radmmm_rowgemm_h3_desc* d);
/* Deferred column sums (ABI 3): a launch with colsum_scratch set and colsum_out == NULL leaves its per-row-tile partial rows
 * in colsum_scratch ([rows][N] floats, rows = the value returned here) and the caller adds them up later -- several launches'
 * finals in one radmmm_colsum_final_multi call.  Returns 0 when this descriptor would take a kernel that cannot leave
 * partials (the generic epilogue, the narrow kernel): give it colsum_out then.  Also 0 for a descriptor without
 * colsum_scratch or one that radmmm_rowgemm_h3 would refuse.  Host only, like radmmm_rowgemm_h3_plan. */
int radmmm_rowgemm_h3_colsum_rows(const radmmm_rowgemm_h3_desc* d);
typedef struct { const float* part; float* out; int nparts; int cols; } radmmm_cs_item;
/* out[c] = sum_p part[p * cols + c] for every item (fixed order per item: deterministic), any number of items */
int radmmm_colsum_final_multi(const radmmm_cs_item* items, int n, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Weight-gradient GEMM (contraction over frames), fp32 MFMA:
 *   P[split][tap][m][n] = sum_{r in split} GY[r, m] * Xm[r + shift(tap), n]
 * m < Mc (out channels), n < Nc (in channels); Xm masked as in radmmm_rowgemm_f32.
 * `splits` partial slabs are written (deterministic; the consumer sums them),
 * P slab layout [taps][Mc][ldp].  Replaces conv weight-gradients of autograd
 * (aten::convolution_backward) for common.py:816-835.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  const float* GY; int ldgy;
  const float* X; int ldx;
  float* P; int ldp; int64_t split_stride;  /* floats between slabs */
  int R;                 /* total rows (B*T) */
  int Mc, Nc;
  int taps, dil;
  int T; const int32_t* lens; int x_mask_mode;
  int splits;
} radmmm_wgrad_desc;

int radmmm_wgrad_f32(const radmmm_wgrad_desc* d, radmmm_stream_t stream);

/* Additive entry points of ABI 4, host only: which kernel radmmm_rowgemm_f32 / radmmm_wgrad_f32 would launch for a descriptor,
 * as RADMMM_F32_KERNEL_CODE(family, b_layout, mt, rows); < 0: the descriptor would be refused (same code and
 * radmmm_last_error text as the entry point, whose validation they share).  mt and rows are the tile height / 16 and the rows
 * per tile of the 16-row kernel, 0 for every other family; b_layout is 0 for the weight gradients.  They make no HIP call and
 * dereference no operand pointer (the pointers' alignment and presence is all they look at), so they answer on a machine
 * without a GPU; the entry points take their decision from the same function.  Tests use them to make sure a shape reaches
 * the kernel they mean to test. */
#define RADMMM_F32_FAMILY_GENERIC 1   /* rowgemm_f32_kernel<bl> */
#define RADMMM_F32_FAMILY_ROWS16  2   /* rowgemm16_kernel<mt, bl> */
#define RADMMM_F32_FAMILY_MIX     3   /* rowgemm_mix_kernel<bl> */
#define RADMMM_F32_FAMILY_WGRAD   4   /* wgrad_f32_kernel */
#define RADMMM_F32_FAMILY_WGRAD16 5   /* wgrad16_kernel */
#define RADMMM_F32_KERNEL_CODE(family, bl, mt, rows) ((family) * 1000000 + (bl) * 100000 + (mt) * 1000 + (rows))
int radmmm_rowgemm_f32_plan(const radmmm_rowgemm_desc* d);  /* <0: the descriptor would be refused */
int radmmm_wgrad_f32_plan(const radmmm_wgrad_desc* d);

/* ------------------------------------------------------------------------------------
 * Weight norm fold / unfold  (torch weight_norm dim=0; common.py:173-174,791,813)
 *   forward : W[tap][co][col(ci)] = g[co] * v[co][ci][tap] / ||v[co]||_2 ,
 *             inv_norm[co] = 1/||v[co]||
 *             col(ci) = ci < perm_split ? ci + off_lo : ci - perm_split + off_hi
 *             (columns not hit by col() are left untouched: zero them once)
 *   backward: from `splits` slabs of dL/dW (layout of W) -> dL/dv [co][ci][tap], dL/dg [co] (+ *poison)
 * v is in the reference's checkpoint layout [Cout][Cin][taps].
 * radmmm_weightnorm_bwd picks one of several kernels from the shape and the alignment of its operands; all of them give
 * the same dv and dg up to the order in which the sum over (ci, tap) is added.
 * ------------------------------------------------------------------------------------ */
int radmmm_weightnorm_fwd(const float* v, const float* g, float* W, float* inv_norm,
                          int Cout, int Cin, int taps, int ldw,
                          int perm_split, int off_lo, int off_hi, radmmm_stream_t stream);
int radmmm_weightnorm_bwd(const float* v, const float* g, const float* inv_norm,
                          const float* dW, int splits, int64_t split_stride,
                          float* dv, float* dg,
                          int Cout, int Cin, int taps, int ldw,
                          int perm_split, int off_lo, int off_hi,
                          const float* poison /* optional device scalar added to every dg element: 0, or NaN when the
                                                 pass's incoming gradient was not finite (the split operands clamp NaN / Inf
                                                 to finite values; this puts the non-finite result back where an AMP
                                                 GradScaler or a gradient-norm clip looks for it) */,
                          radmmm_stream_t stream);
/* radmmm_weightnorm_bwd of up to 8 one-tap tensors (taps must be 1) in ONE launch: one workgroup per (item, output
 * channel) running the single call's register kernel, so dv / dg are what n calls of radmmm_weightnorm_bwd write on the same
 * slabs, bit for bit.  `poison` is shared.  Only items of the register path are taken -- Cin a multiple of 4 and <= 2048;
 * perm_split, off_lo, off_hi, ldw, split_stride multiples of 4; 16-byte aligned dW, v, dv -- anything else returns -1
 * ("weightnorm_bwd_multi: ... register path") before any HIP call and is left to per-item calls.  Additive entry point of
 * ABI 4. */
typedef struct radmmm_wnb_item {
  const float* v;
  const float* g;
  const float* inv_norm;
  const float* dW;
  float* dv;
  float* dg;
  int64_t split_stride;
  int splits;
  int Cout, Cin, ldw;
  int perm_split, off_lo, off_hi;
} radmmm_wnb_item;
int radmmm_weightnorm_bwd_multi(const radmmm_wnb_item* items, int n, int taps, const float* poison, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * WN input assembly (cat((z0, context), 1), common.py:819) in channels-last, K-padded:
 *   X0[r, 0:D] = ctx[r, 0:D] ; X0[r, D:D+h] = z[r, 0:h] ; X0[r, D+h:ldx0] = 0
 * and its gradient scatter:
 *   gctx[r, 0:D] (+)= gX0[r, 0:D] ; gz[r, 0:h] += gX0[r, D:D+h]
 * Columns beyond these ranges (gctx[r, D:ldctx], gz[r, h:ldz]) are never written.
 * ------------------------------------------------------------------------------------ */
int radmmm_wn_input_fwd(const float* ctx, int ldctx, const float* z, int ldz,
                        float* X0 /* may be NULL when the split copy is written (ABI 3) */, int ldx0, int rows, int D, int h,
                        void* X0h, void* X0l /* optional split copy, pitch ldx0, may be NULL */,
                        const radmmm_split_opts* so, radmmm_stream_t stream);
int radmmm_wn_input_bwd(const float* gX0, int ldx0, float* gctx, int ldctx, int ctx_accum,
                        float* gz, int ldz, int rows, int D, int h, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Squeeze = nn.Unfold(kernel=(g,1), stride=g) of the reference (decoders.py:118-122,178; models/radmmm.py:114-120)
 * straight from the reference layout into channels-last rows of a wider matrix:
 *   out[(b*T' + t') * ld + col0 + c*g + k] = in[(b*C + c)*T + t'*g + k],  T' = T / g (frames beyond g*T' are dropped)
 * so the flow variable and the context LSTM's input are assembled without a permuted copy or a concatenation.
 * radmmm_unsqueeze_rows is its gradient: gin[b, c, t] = gout[row(t / g)][col0 + c*g + t % g] for t < g*T', else 0.
 * g must divide 64.
 * ------------------------------------------------------------------------------------ */
int radmmm_squeeze_rows(const float* in /* [B, C, T] */, float* out, int B, int C, int T, int g, int ld, int col0,
                        radmmm_stream_t stream);
int radmmm_unsqueeze_rows(const float* gout, float* gin /* [B, C, T] */, int B, int C, int T, int g, int ld, int col0,
                          radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Affine coupling (AffineTransformationLayer.forward, common.py:1163-1185):
 *   su = O[r, 0:h], b = O[r, h:2h]; (s, log_s) = scaling(su)
 *   zout[r, 0:h] = z[r, 0:h]; zout[r, h:2h] = s * z[r, h:2h] + b; zout[r, 2h:ldz] = z[...]
 *   log_s[r, 0:h] stored with row stride h.
 * backward: given gzout, glog_s (may be NULL), O, z:
 *   gO[r, 0:h] = (gzout1 * z1 + glog_s * dlog_s/ds) * ds/dsu ; gO[r, h:2h] = gzout1
 *   gz[r, 0:h] = gzout[r, 0:h]; gz[r, h:2h] = gzout1 * s ; gz[r, 2h:ldz] = gzout[...]
 * gO[r, 2h:ldo] is never written.
 * ------------------------------------------------------------------------------------ */
int radmmm_affine_coupling_fwd(const float* O, int ldo, const float* z, int ldz,
                               float* zout, float* log_s, int rows, int h, int scaling,
                               radmmm_stream_t stream);
int radmmm_affine_coupling_bwd(const float* O, int ldo, const float* z, int ldz,
                               const float* gzout, const float* glog_s,
                               float* gO, float* gz, int rows, int h, int scaling,
                               radmmm_stream_t stream);

/* y[r, c] = g[r, c] * act'(saved[r, c]) * w(r), c < cols: derivative of the activation from its
 * saved OUTPUT (dact 0: none, saved may be NULL) times a row weight (rowscale 0: 1; 1: mask;
 * 2: mask * partial-conv ratio of a (taps, dil) window) -- the step from dL/d(act output) to
 * dL/d(conv accumulator) of ConvNorm/PartialConv1d (common.py:179-191) */
int radmmm_dact_mul(const float* g, int ldg, const float* saved, int lds, float* y, int ldy,
                    int rows, int cols, int dact, int rowscale, int T, const int32_t* lens,
                    int taps, int dil,
                    void* yh, void* yl, int ldyh, float yscale /* optional split-fp16 copy of yscale*y */,
                    const radmmm_split_opts* so /* NULL: f16 pair, no flag */, radmmm_stream_t stream);

/* out[c] = sum_r w(r) * f(X[r, c]), f = identity or square;  row_weight 0: 1 ; 1: [t < lens[b]] ;
 * 2: (cnt+1e-6)/taps over valid rows (undoes the partial-conv ratio: bias gradient of
 * PartialConv1d).  Also the masked first/second moments of MaskedBatchNorm1d
 * (maskedbatchnorm1d.py:83-84).                                                          */
int radmmm_colsum(const float* X, int ldx, float* out, float* scratch, int rows, int cols,
                  int row_weight, int T, const int32_t* lens, int taps, int dil, int square,
                  radmmm_stream_t stream);
int64_t radmmm_colsum_scratch_floats(int rows, int cols);

/* ------------------------------------------------------------------------------------
 * Flow NLL reductions (compute_flow_loss, loss.py:85-110) on arbitrary-stride
 * [B, C, T] views:  mode 0: sum(x*m), mode 1: sum((x*m)^2);   m = [t < lens[b]].
 * Deterministic two-stage reduction; `out` receives one float.
 * backward (elementwise): gx[b,c,t] = coef[0] * m * (mode 1 ? 2*x : 1); gx uses x's strides
 * ------------------------------------------------------------------------------------ */
int radmmm_masked_reduce(const float* x, int B, int C, int T, int64_t sb, int64_t sc, int64_t st,
                         const int32_t* lens, int mode, float* out, float* scratch,
                         radmmm_stream_t stream);
int64_t radmmm_masked_reduce_scratch_floats(int B, int C, int T);
int radmmm_masked_reduce_bwd(const float* x, int B, int C, int T, int64_t sb, int64_t sc,
                             int64_t st, const int32_t* lens, int mode, const float* coef,
                             float* gx, radmmm_stream_t stream);

/* fused_add_tanh_sigmoid_multiply (common.py:66-73): y[r, c] = tanh(a+b)[r, c] *
 * sigmoid(a+b)[r, n + c], c < n.  Not on any config's path (WaveNetOriginal only). */
int radmmm_fused_add_tanh_sigmoid_multiply(const float* a, const float* b, int ld, float* y,
                                           int ldy, int rows, int n, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Piecewise-quadratic spline coupling transform (splines.py:241-339, forward branch)
 * on x [rows, h] (already normalised to [0,1) by (z+bound)/(2 bound)), q [rows, h*(2K+1)]
 * channels-last with channel index c*(2K+1)+j (first K: widths, last K+1: heights).
 *   y [rows, h], logj_sum[0:rows] = sum_c logj; logj_sum must have room for rows + rows*h
 *   floats (the tail receives the per-element log-jacobians the sums are reduced from)
 * backward: gy [rows,h], glogj [rows] -> gx [rows,h], gq [rows, h*(2K+1)]
 * ------------------------------------------------------------------------------------ */
int radmmm_pq_spline_fwd(const float* x, int ldx, const float* q, int ldq, float* y, int ldy,
                         float* logj_sum, int rows, int h, int K, radmmm_stream_t stream);
/* INDEX accounting of the forward bin search (splines.py:300-306 `searchsorted`), for parity tests: bins[r*h + c] = the bin
 * radmmm_pq_spline_fwd picks for element (r, c), or -1 for an element outside [0, 1) (passed through); edge_l / edge_r = the
 * two edges of that bin as the search compared them (the kernel's running sum of the softmax widths; 1 for the last bin). */
int radmmm_pq_spline_bins(const float* x, int ldx, const float* q, int ldq, int32_t* bins, float* edge_l, float* edge_r,
                          int rows, int h, int K, radmmm_stream_t stream);
/* inverse direction of the same transform (splines.py:327-339; no log-jacobian): x from y, both in [0,1) units */
int radmmm_pq_spline_inv(const float* y, int ldy, const float* q, int ldq, float* x, int ldx, int rows, int h, int K,
                         radmmm_stream_t stream);
int radmmm_pq_spline_bwd(const float* x, int ldx, const float* q, int ldq, const float* gy,
                         int ldgy, const float* glogj, float* gx, int ldgx, float* gq, int ldgq,
                         int rows, int h, int K, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * FiLM residual block tail (FiLMResBlock.forward, common.py:728-735) with the training-mode
 * masked batch-norm (maskedbatchnorm1d.py:53-118) fused in, channels-last [rows, C]:
 *   y = use_bn ? (h2 - mean) * invstd * w + b : h2 ;  t = y * (c1[:, 0:C] + 1) + c1[:, C:2C]
 *   out = 0.5 * (leaky_relu(t) + x1r)
 * mean/invstd are the caller's masked statistics (radmmm_colsum with square = 0/1).
 * backward: gout -> gh2, gc1 [rows, 2C], gx1r, and dL/dw, dL/db of the batch-norm affine;
 * n_valid = number of unmasked frames; scratch: radmmm_film_bwd_scratch_floats(rows, C).
 * radmmm_film_bwd's use_bn: 0 = no batch-norm, 1 = mean/invstd are the masked statistics of this h2 (training mode: gh2
 * carries their derivatives), 2 = mean/invstd are constants (eval mode, running statistics: gh2 = invstd * w * g_y;
 * dL/dw, dL/db are the same column sums in both).
 * ------------------------------------------------------------------------------------ */
int radmmm_film_fwd(const float* h2, int ldh, const float* c1, int ldc, const float* x1r, int ldx,
                    const float* mean, const float* invstd, const float* w, const float* b,
                    float* out, int ldo, int rows, int C, int use_bn, radmmm_stream_t stream);
int radmmm_film_bwd(const float* h2, int ldh, const float* c1, int ldc, const float* gout, int ldg,
                    const float* mean, const float* invstd, const float* w, const float* b,
                    float n_valid, int T, const int32_t* lens, float* gh2, int ldgh, float* gc1,
                    int ldgc, float* gx1r, int ldgx, float* gw, float* gb, float* scratch, int rows,
                    int C, int use_bn, radmmm_stream_t stream);
int64_t radmmm_film_bwd_scratch_floats(int rows, int C);
/* radmmm_film_bwd in two halves, for synchronised masked batch-norm statistics under data parallelism
 * (maskedbatchnorm1d.py:88-95; MaskedBatchNorm1d.distributed_sync, tts_lightning_modules.py:238-243): _sums leaves this
 * rank's S = [sum g_y | sum g_y xhat] ([2][C]) at scratch + ceil(rows/64)*2*C ... (radmmm_film_bwd_scratch_floats - 2*C)
 * and copies it to gb / gw; the caller all-reduces S in place; _apply uses it with n_valid = the global frame count. */
int radmmm_film_bwd_sums(const float* h2, int ldh, const float* c1, int ldc, const float* gout, int ldg,
                         const float* mean, const float* invstd, const float* w, const float* b, float* gw, float* gb,
                         float* scratch, int rows, int C, radmmm_stream_t stream);
int radmmm_film_bwd_apply(const float* h2, int ldh, const float* c1, int ldc, const float* gout, int ldg,
                          const float* mean, const float* invstd, const float* w, const float* b, float n_valid, int T,
                          const int32_t* lens, float* gh2, int ldgh, float* gc1, int ldgc, float* gx1r, int ldgx,
                          const float* scratch, int rows, int C, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Alignment attention (ConvAttention.forward, common.py:1262-1277), from projected
 * queries Q [B, T1, Ca] and keys Kx [B, T2, Ca] (channels-last):
 *   d[b,t,s] = -temp * sum_c (Q[b,t,c]-K[b,s,c])^2
 *   logprob = log_softmax_s(d) + log(prior + 1e-8)   (prior NULL: logprob = d)
 *   attn = softmax_s(logprob masked to s < in_lens[b])
 * outputs attn, logprob [B, T1, T2].  backward: gattn, glogprob -> gQ, gK.
 * ------------------------------------------------------------------------------------ */
int radmmm_attn_fwd(const float* Q, const float* Kx, const float* prior, const int32_t* in_lens,
                    float* attn, float* logprob, int B, int T1, int T2, int Ca, float temp,
                    radmmm_stream_t stream);
int radmmm_attn_bwd(const float* Q, const float* Kx, const float* prior, const int32_t* in_lens,
                    const float* attn, const float* logprob, const float* gattn,
                    const float* glogprob, float* gQ, float* gK, float* gd_scratch /* B*T1*T2 */,
                    int B, int T1, int T2, int Ca, float temp, radmmm_stream_t stream);

/* Monotonic alignment search, width 1 (alignment.py:31-59; INTEGER/INDEX path, bit-exact
 * given identical log inputs).  logp [B, T1, T2] = log(attn) (caller's log), per item the
 * [out_lens[b], in_lens[b]] corner is aligned; hard [B, T1, T2] receives 0/1 (zeroed
 * outside).  scratch: radmmm_mas_scratch_bytes(B, T1, T2). */
int radmmm_mas_width1(const float* logp, const int32_t* in_lens, const int32_t* out_lens,
                      float* hard, void* scratch, int B, int T1, int T2, radmmm_stream_t stream);
/* Same search on PROBABILITIES attn [B, T1, T2] (TTSModel.binarize_attention, tts_lightning_modules.py:270-284,
 * hands alignment.py:31 the soft attention and the log is taken inside, alignment.py:36): the kernel takes the log
 * itself, correctly rounded to fp32 (a first launch over the whole chip, into `scratch`; the search itself is a chain
 * of T1 dependent steps per utterance and keeps nothing but an LDS row exchange and a ballot in each). */
int radmmm_mas_width1_prob(const float* attn, const int32_t* in_lens, const int32_t* out_lens,
                           float* hard, void* scratch, int B, int T1, int T2, radmmm_stream_t stream);
int64_t radmmm_mas_scratch_bytes(int B, int T1, int T2);

/* STFT magnitude -> mel -> log-clamp (audio_processing.py:137-154, 227-255).
 * audio [B, S]; basis [2*(n_fft/2+1)][n_fft] windowed DFT rows (re then im);
 * mel_basis [n_mel][n_fft/2+1]; out mel [B, n_mel, 1 + S/hop] (reference layout). */
int radmmm_stft_mel(const float* audio, const float* basis, const float* mel_basis, float* mel,
                    float* scratch, int B, int S, int n_fft, int hop, int n_mel,
                    float clip, radmmm_stream_t stream);
int64_t radmmm_stft_mel_scratch_floats(int B, int S, int n_fft, int hop, int n_mel);

/* ------------------------------------------------------------------------------------
 * Split-f16 support (radmmm_rowgemm_h3's operands): fp32-class GEMM on the f16 matrix
 * cores by operand splitting (x*scale = hi + lo in fp16; A.B ~= Ah.Bh + Ah.Bl + Al.Bh with fp32
 * accumulate).  radmmm_split_f16 writes hi/lo [rows][ldh] halves (ldh % 8 == 0, zero padded).
 * See DESIGN.md §4.2 for the measured rate and error.
 * ------------------------------------------------------------------------------------ */
int radmmm_split_f16(const float* x, int ld, void* hi, void* lo, int ldh, int rows, int cols,
                     float scale, const radmmm_split_opts* so, radmmm_stream_t stream);
/* weight-norm fold (see radmmm_weightnorm_fwd) straight into split packed weights
 * W{h,l}[tap][Cout][ldk] = split(scale * g v/||v||); g == NULL: plain weights (inv_norm unused).
 * so->fmt RADMMM_SPLIT_X8B: Wl is the B-role cross array (ldk % 32 == 0) */
int radmmm_weightnorm_fwd_h3(const float* v, const float* g, void* Wh, void* Wl, float* inv_norm,
                             int Cout, int Cin, int taps, int ldk, int perm_split, int off_lo,
                             int off_hi, float scale, const radmmm_split_opts* so, radmmm_stream_t stream);
/* dst[b][c][r] = src[b][r][c] for both members of a split pair (batches of [rows][cols]); fmt RADMMM_SPLIT_X8B:
 * src_l / dst_l are B-role cross arrays (their 8-bit hi parts are re-derived from the fp16 hi, the 8-bit lo parts
 * move with the transposition; ld_src, ld_dst % 32 == 0, x8_exp as the source was written) */
int radmmm_transpose_f16_pair(const void* src_h, const void* src_l, int ld_src, int64_t src_batch,
                              void* dst_h, void* dst_l, int ld_dst, int64_t dst_batch, int batches,
                              int rows, int cols, int fmt, int x8_exp, radmmm_stream_t stream);
/* The two above for up to 16 tensors in ONE launch each: the weights of a flow step are mostly 4 - 9 MB, where a launch of its
 * own is two memory round trips long rather than bandwidth-bound.  Same arithmetic per tensor, same results. */
typedef struct radmmm_wn_item {
  const float* v;
  const float* g;       /* NULL: plain weights */
  void* Wh;
  void* Wl;
  float* inv_norm;      /* may be NULL when g is NULL */
  int Cout, Cin, taps, ldk, perm_split, off_lo, off_hi;
} radmmm_wn_item;
int radmmm_weightnorm_fwd_h3_multi(const radmmm_wn_item* items, int n, float scale, const radmmm_split_opts* so,
                                   radmmm_stream_t stream);
typedef struct radmmm_tp_item {
  const void* src_h;
  const void* src_l;
  void* dst_h;
  void* dst_l;
  int64_t src_batch, dst_batch;
  int ld_src, ld_dst, batches, rows, cols;
} radmmm_tp_item;
/* (8-bit B-role pairs only: fmt RADMMM_SPLIT_X8B) */
int radmmm_transpose_f16_pair_multi(const radmmm_tp_item* items, int n, int fmt, int x8_exp, radmmm_stream_t stream);
/* Workgroup slots the GEMM grids are sized for: the device's CU count, or RADMMM_GEMM_CUS (32 .. CUs; read once
 * per process) when data-parallel runs leave CUs to RCCL's channel kernels (Lightning `strategy: ddp`,
 * configs/RADMMM_train_config.yaml:28; rad_mmm_amd/ddp.py reserve_collective_cus). */
int radmmm_gemm_cu_slots(void);
/* ------------------------------------------------------------------------------------
 * CTC loss of the alignment attention (loss.py:112-141: torch.nn.CTCLoss, blank 0, zero_infinity, with the targets
 * 1, 2, .., L_b -- every text position once, in order) for a whole batch, value and gradient in one call (two launches, no host read).
 *   lp [B][T][C] log-probabilities (log-softmax outputs, class 0 = blank), lens_txt[b] = L_b <= C - 1, lens_mel[b] = T_b <= T
 *   nll [B]: -log p(targets | frames 0 .. T_b - 1), or 0 where no alignment exists (T_b < L_b)
 *   grad [B][T][C]: d nll[b] / d lp as torch's ctc_loss_backward defines it (exp(lp) - exp(log-sum alpha*beta + nll - lp);
 *   0 for frames >= T_b and for utterances without alignment)
 *   scratch: radmmm_ctc_monotonic_scratch_floats(B, T, C) floats.  At most 511 text positions.
 * ------------------------------------------------------------------------------------ */
int64_t radmmm_ctc_monotonic_scratch_floats(int B, int T, int C);
int radmmm_ctc_monotonic(const float* lp, const int32_t* lens_txt, const int32_t* lens_mel, float* nll, float* grad,
                         float* scratch, int B, int T, int C, radmmm_stream_t stream);

/* A HIP stream whose kernels may use only `enabled_cus` of the device's CUs (hipExtStreamCreateWithCUMask); *out receives
 * the hipStream_t (wrap it, e.g. torch.cuda.ExternalStream).  radmmm_stream_destroy releases it. */
int radmmm_stream_create_masked(int enabled_cus, void** out);
int radmmm_stream_destroy(void* stream);

/* Weight gradient on the split-f16 path.  Operands are transposed, time-contiguous, zero-gapped
 * split copies made by radmmm_transpose_split_act from channels-last fp32 [B*T][ld]:
 *   out[c][front + b*Tp + t] = split(scale * x[b*T+t][c]),  t < (mask_mode ? lens[b] : T), else 0
 * (Tp >= T + max|shift|, front >= max|shift|, ldk % 8 == 0, ldk >= front + B*Tp; the front columns
 * and the row tail must be zero: allocate zeroed once, the gaps are rewritten on every call).
 * o1h/o1l (optional) receive the copy advanced by one column, used for odd tap shifts.
 *   P[split][tap][m][n] = acc_scale * sum_k GYt[m][k] * Xt[n][k + (tap - taps/2)*dil]
 * over the Kt (% 32 == 0) columns k in [k0, k0 + Kt), k0 = front; split-K into `splits` slabs as
 * radmmm_wgrad_f32.  ldk >= k0 + Kt + max|shift|. */
int radmmm_transpose_split_act(const float* x, int ld, int C, int B, int T, int Tp, int front,
                               const int32_t* lens, int mask_mode, float scale, void* oh, void* ol,
                               void* o1h, void* o1l, int ldk, radmmm_stream_t stream);
/* radmmm_transpose_split_act + the weighted column sums of x (bias gradient) from the same pass:
 * part [B * ceil(Tp / 64)][C] partial rows, to be added by radmmm_colsum_final(part, out, nparts, C).
 * sum_weight / sum_taps / sum_dil as radmmm_colsum's row_weight / taps / dil. */
int radmmm_transpose_split_act_colsum(const float* x, int ld, int C, int B, int T, int Tp, int front,
                                      const int32_t* lens, int mask_mode, float scale, void* oh, void* ol, void* o1h,
                                      void* o1l, int ldk, float* part, int sum_weight, int sum_taps, int sum_dil,
                                      radmmm_stream_t stream);
int radmmm_colsum_final(const float* part, float* out, int nparts, int cols, radmmm_stream_t stream);
/* y = g * act'(saved) (radmmm_dact_mul without row weights) written three ways in one pass, with no fp32 copy of y:
 * the row-major split pair yh/yl [rows][ldyh] of scale*y in so's format (feeds the data-gradient GEMM), the transposed
 * zero-gapped split-f16 pair oh/ol [C][ldk] of scale*y (radmmm_transpose_split_act's layout: feeds radmmm_wgrad_h3), and
 * the column sums of y as part [B * ceil(Tp / 64)][C] (radmmm_colsum_final adds them: the bias gradient).
 * C, ldg, lds multiples of 4; yh may be NULL. */
int radmmm_dact_mul_transposed(const float* g, int ldg, const float* saved, int lds, int C, int B, int T, int Tp,
                               int front, int dact, float scale, void* yh, void* yl, int ldyh,
                               const radmmm_split_opts* so, void* oh, void* ol, int ldk, float* part,
                               radmmm_stream_t stream);
/* radmmm_dact_mul for a backward that needs no fp32 copy of y: y = g * act'(saved) * row factor (rowscale as radmmm_dact_mul:
 * 0 none, 1 the length mask, 2 mask x partial-conv ratio, partialconv1d.py:75-81) written as the row-major split pair
 * yh/yl [B*T][ldyh] of scale*y only, and the BIAS-gradient sums in the same pass: part [B * ceil(T / 64)][C] partial rows of
 * sum_t g * act' * [t < len] (= radmmm_colsum(y, row_weight = rowscale): the ratio and its inverse weight cancel), to be
 * added by radmmm_colsum_final.  C, ldg, lds multiples of 4, 16-byte aligned g / saved. */
int radmmm_dact_mul_rows(const float* g, int ldg, const float* saved, int lds, int C, int B, int T, int dact,
                         int rowscale, const int32_t* lens, int taps, int dil, float scale, void* yh, void* yl,
                         int ldyh, const radmmm_split_opts* so, float* part, radmmm_stream_t stream);
/* y_j = g * act'(saved_j), j < n <= 4, in ONE pass over g (the four res/skip layers of a WN all start from the gradient of the
 * skip sum, common.py:816-835): per item the row-major split pair yh / yl (pitch ldyh, format / exponent / saturation flag from
 * `so`; ylo16: the optional fp16 lo part beside an 8-bit cross array) and B * ceil(T / 64) rows of column-sum partials (pitch
 * C) for radmmm_colsum_final(_multi) -- element for element what n calls of radmmm_dact_mul_rows with rowscale 0 write.
 * All saved tensors share the pitch lds; so->lo16 is ignored (per item). */
typedef struct radmmm_dact_item {
  const float* saved;
  void* yh;
  void* yl;
  void* ylo16; /* or NULL */
  float* part;
} radmmm_dact_item;
int radmmm_dact_mul_rows_multi(const float* g, int ldg, const radmmm_dact_item* items, int n, int lds, int C, int B, int T,
                               int dact, float scale, int ldyh, const radmmm_split_opts* so, radmmm_stream_t stream);
/* number of workgroup tiles radmmm_wgrad_h3 launches per split (the caller picks `splits` so that
 * tiles * splits fills whole rounds of the CUs: one workgroup per CU) */
int radmmm_wgrad_h3_tiles(int Mc, int Nc, int taps);
int radmmm_wgrad_h3(const void* GYh, const void* GYl, const void* Xh, const void* Xl, const void* X1h,
                    const void* X1l, int ldk, int k0, int Kt, float* P, int ldp, int64_t split_stride, int Mc,
                    int Nc, int taps, int dil, int splits, float acc_scale, int nprod /* 3 or 1, as radmmm_rowgemm_h3_desc */,
                    radmmm_stream_t stream);

/* The same weight gradient on ROW-MAJOR split operands (csrc/wgrad_rm.hip): GYh/GYl [R][ldg] and Xh/Xl [R][ldx] are the
 * [frames][channels] fp16 hi/lo pairs the GEMM epilogues write (R = B*T rows, utterance-major), contracted over the frames
 * with the transposition done in the LDS read; no transposed copies.
 *   P[split][tap][m][n] = acc_scale * sum_f GY[f][m] * X[f + s][n],  s = (tap - taps/2)*dil, for f + s in f's utterance.
 * x_mask: X rows at frames >= lens[b] count as zeros (partial padding: the conv's input is x * mask).  ldg, ldx %% 8 == 0,
 * 16-byte aligned operands, T >= 32, at most 1024 utterances; ldp >= Nc; slabs `split_stride` floats apart;
 * radmmm_wgrad_rm_tiles as radmmm_wgrad_h3_tiles. */
int radmmm_wgrad_rm_tiles(int Mc, int Nc, int taps);
int radmmm_wgrad_rm(const void* GYh, const void* GYl, int ldg, const void* Xh, const void* Xl, int ldx, int R, int T,
                    const int32_t* lens, int x_mask, float* P, int ldp, int64_t split_stride, int Mc, int Nc, int taps,
                    int dil, int splits, float acc_scale, radmmm_stream_t stream);

/* The same weight gradient under the FP8-cross scheme (csrc/wgrad_rm8.hip; common.py:816-835 backward,
 * partialconv1d.py:82): GYh.Xh on the f16 matrix pipe + both cross terms GYh.Xl + GYl.Xh in one block-scaled FP8 MFMA per
 * 32-frame K step -- two thirds of radmmm_wgrad_rm's MFMA work.  GYx / Xx are the tensors' 8-bit cross arrays
 * (RADMMM_SPLIT_X8A, written with exponents g8_exp / x8_exp); only their lo8 halves are read, the hi8 parts are derived
 * from the fp16 hi planes in registers.  No fp16 lo array is involved.  ldg, ldx multiples of 32. */
int radmmm_wgrad_rm8(const void* GYh, const void* GYx, int ldg, int g8_exp, const void* Xh, const void* Xx, int ldx, int x8_exp,
                     int R, int T, const int32_t* lens, int x_mask, float* P, int ldp, int64_t split_stride, int Mc, int Nc,
                     int taps, int dil, int splits, float acc_scale, radmmm_stream_t stream);

/* The same weight gradient on ONE product: GYh . Xh alone, on the f16 matrix pipe (csrc/wgrad_rm8.hip, the one-product
 * instantiation of radmmm_wgrad_rm8's kernel).  For weight gradients that are leaves of the step: the operands are the
 * fp16 hi planes only, so each operand carries a relative rounding of at most 2^-11 and an element of P differs from the
 * exact contraction by at most 2^-10 * sum_f |GY||X| (plus the fp32 accumulation); over thousands of frames the
 * roundings average out (profiles/wgrad_one_pass_emulation.txt).  Tiles, tile order, split-K ranges, masks, tap shifts
 * and the accumulation order are radmmm_wgrad_rm8's: the slabs differ from that function's by its cross terms only.
 * GYh [R][ldg] / Xh [R][ldx] as there; ldg, ldx multiples of 32, 16-byte aligned operands, T >= 32, at most 1024
 * utterances, splits >= 1, radmmm_wgrad_rm_tiles tiles.  Bad arguments return -1 before any HIP call. */
int radmmm_wgrad_rmh(const void* GYh, int ldg, const void* Xh, int ldx, int R, int T, const int32_t* lens, int x_mask, float* P,
                     int ldp, int64_t split_stride, int Mc, int Nc, int taps, int dil, int splits, float acc_scale,
                     radmmm_stream_t stream);

/* radmmm_wgrad_rmh / radmmm_wgrad_rm with a frame-shift origin and column origins:
 *   P[split][tap][m][n] = acc_scale * sum_f GY[f][g_col0 + m] * X[f + shift0 + s][x_col0 + n],  s = (tap - taps/2)*dil,
 * over the frames f whose partner f + shift0 + s lies in f's own utterance (and, with x_mask, below its length): with
 * taps = 1 and shift0 = -1 / +1, X read this way is the previous / next frame's row with zeros across the utterance
 * boundary -- the h_prev operand of an LSTM's recurrent weight gradient (dW_hh[d] = dG_d^T h_prev) taken from y itself.
 * The pointers are the BASE pointers of planes of exactly R rows of ldg / ldx halves; the Mc / Nc channels start at column
 * g_col0 / x_col0 of a row (multiples of 8, g_col0 + Mc <= ldg, x_col0 + Nc <= ldx), and no read goes beyond the planes.
 * Largest shift0: the mask rule holds for any shift (a row is tested against its own utterance); what bounds it is the
 * 32-bit offset arithmetic, (R + 96 + |shift0| + (taps/2)*dil) * ldx * 2 < 2^31 (csrc/common.h, wgrad_rm_shift_fits).
 * Tiles, split-K ranges and K order are those of the plain entry points, whose results these reproduce bit for bit on
 * operands shifted by hand (shift0 = 0 and zero origins: the plain entry points themselves).  Bad arguments return -1
 * before any HIP call. */
int radmmm_wgrad_rmh_shift(const void* GYh, int ldg, int g_col0, const void* Xh, int ldx, int x_col0, int shift0, int R, int T,
                           const int32_t* lens, int x_mask, float* P, int ldp, int64_t split_stride, int Mc, int Nc, int taps,
                           int dil, int splits, float acc_scale, radmmm_stream_t stream);
int radmmm_wgrad_rm_shift(const void* GYh, const void* GYl, int ldg, int g_col0, const void* Xh, const void* Xl, int ldx, int x_col0,
                          int shift0, int R, int T, const int32_t* lens, int x_mask, float* P, int ldp, int64_t split_stride,
                          int Mc, int Nc, int taps, int dil, int splits, float acc_scale, radmmm_stream_t stream);

/* Up to 8 one-product weight gradients (radmmm_wgrad_rmh_shift jobs) as ONE launch: the jobs share R, T, taps, dil, lens /
 * x_mask, shift0, splits and acc_scale; each owns its operands, column origins, extents and slabs.  Job k contributes
 * radmmm_wgrad_rm_tiles(Mc, Nc, taps) * splits workgroups, laid out one job after the other; a workgroup finds its job through
 * a table of first tiles in the kernel arguments and from there runs the single launch's code with that job's values: the
 * tiles of a job are decoded as a launch of that job alone with the same `splits` decodes them, and its slabs are those
 * launches' slabs bit for bit.  For contractions whose operands are ready at the same moment and whose single launches are
 * too short to fill the machine without a large split factor (the four res/skip 1x1 convs of a WN: 64 tiles, splits 4,
 * instead of four launches of 16 tiles with splits 15 -- a quarter of the slab traffic).  Every job must pass
 * radmmm_wgrad_rmh_shift's checks; 1 <= n <= 8.  Bad arguments return -1 before any HIP call.  Additive entry point of
 * ABI 4. */
typedef struct radmmm_wg_item {
  const void* GYh; /* base of the [R][ldg] fp16 hi plane */
  const void* Xh;  /* base of the [R][ldx] fp16 hi plane */
  float* P;        /* slabs [splits][taps][Mc][ldp], split_stride floats apart */
  int64_t split_stride;
  int ldg, g_col0;
  int ldx, x_col0;
  int Mc, Nc;
  int ldp;
} radmmm_wg_item;
int radmmm_wgrad_rmh_group(const radmmm_wg_item* items, int n, int shift0, int R, int T, const int32_t* lens, int x_mask, int taps,
                           int dil, int splits, float acc_scale, radmmm_stream_t stream);

/* fp16 hi (and, unless lo is NULL, lo) planes of `groups` column groups of x [rows][ld]: group g holds columns
 * [g * gcols, (g + 1) * gcols) of x, scaled, at columns [g * gpitch, g * gpitch + gcols) of hi / lo [rows][ldh]; every other
 * column of the planes is written as zero.  The bits of radmmm_split_f16 (RADMMM_SPLIT_F16) per element; sat_flag (or
 * NULL) as there.  gpitch, ldh multiples of 8, groups * gpitch <= ldh, gcols <= gpitch, groups * gcols <= ld.  One pass
 * gives both directions of an LSTM's y [rows][2H] their own 16-byte aligned group for radmmm_wgrad_rm*_shift. */
int radmmm_split_f16_groups(const float* x, int ld, void* hi, void* lo, int ldh, int rows, int gcols, int groups, int gpitch,
                            float scale, int* sat_flag, radmmm_stream_t stream);

/* Bidirectional single-layer LSTM, recurrent part (reference: the decoder's context LSTM,
 * models/radmmm.py:141-146 = torch.nn.LSTM(bidirectional, batch_first) on a packed batch; gate order
 * i, f, g, o; frames t >= lens[b] produce h = c = 0 as pad_packed_sequence does).
 *   G  [B*T][8H]  in: x W_ih^T + b_ih + b_hh (direction d in columns d*4H ..); out: gate activations
 *   W_hh [2][4H][H];  y, c [B*T][2H];  scratch sizes: radmmm_lstm_scratch_bytes(B, H, which) with
 *   which = 0 wsplit, 1 hsplit (fwd), 2 wtpack, 3 P, 4 dcbuf (bwd).
 * radmmm_lstm_bwd overwrites G with the pre-activation gradients dG; the input / weight / bias
 * gradients are plain GEMMs of dG (dW_ih = dG^T x, dx = dG W_ih, db = colsum dG, dW_hh[d] = dG_d^T h_prev).
 * gscale: ignored, may be NULL.  (Until this revision of ABI 4 it was a device scalar that brought dG into fp16 range;
 * the kernel now gives every batch row of its fp16 operand its own power-of-two scale per step, so no gradient range or
 * growth along the recurrence is clamped.  The parameter stays so that existing callers keep working.)
 * All T steps run in ONE launch when the grid (ceil(H/8) x 2 x ceil(B/32) workgroups) fits one workgroup per CU: the
 * workgroups hand h / the partial recurrent gradients from step to step through memory, the data being its own ready
 * flag (csrc/lstm.hip).  The forward pass then needs hseq, radmmm_lstm_hseq_bytes(B, T, H) bytes of scratch (one operand
 * slot per step); that function returns 0, and hseq may be null, when the dimensions take the launch-per-step path. */
int64_t radmmm_lstm_scratch_bytes(int B, int H, int which);
int64_t radmmm_lstm_hseq_bytes(int B, int T, int H);
int radmmm_lstm_fwd(float* G, const float* W_hh, float* y, float* c, const int32_t* lens, void* wsplit, void* hsplit,
                    void* hseq, int B, int T, int H, radmmm_stream_t stream);
int radmmm_lstm_bwd(float* G, const float* c, const float* dy, const float* W_hh, const int32_t* lens, void* wtpack,
                    float* P, float* dcbuf, int B, int T, int H, const float* gscale, radmmm_stream_t stream);
/* Additive entry point of ABI 4, read-only: the form the calling thread's last radmmm_lstm_fwd (which = 0) /
 * radmmm_lstm_bwd (which = 1) ran in -- 1 = one launch per step, 2 = single cooperative launch, 0 = no call yet.  It is
 * recorded where the launch decision is made, including a refused cooperative launch that falls through to per-step. */
int radmmm_lstm_last_path(int which);

/* Channel-mix matrix of the LUS invertible 1x1 conv (common.py:507-548, Invertible1x1ConvLUS.forward's
 * W = P (L U) with L = tril(lower,-1) + diag(lower_diag), U = triu(upper,1) + diag(upper_diag), and
 * log|det W| = sum log|upper_diag|) in one launch each way instead of ~16 small stock launches.
 * P, lower, upper: row-major fp32 [c][c]; c <= 256.  fwd writes the whole zero-padded [ldw][ldw] matrix W
 * with the c x c block at rows [0,c), columns [col_offset, col_offset+c) (what the flow step's first GEMM
 * reads; an early exit is a column offset) and the scalar logdet (may be NULL).  bwd reads the same
 * block of gW [ldw][ldw] and the device scalar g_logdet (may be NULL) and writes the full [c][c]
 * g_lower (strictly lower, zeros elsewhere), g_upper (strictly upper) and g_upper_diag [c]. */
int radmmm_lu_weight_fwd(const float* P, const float* lower, const float* lower_diag, const float* upper,
                         const float* upper_diag, int c, float* W, int ldw, int col_offset, float* logdet,
                         radmmm_stream_t stream);
int radmmm_lu_weight_bwd(const float* P, const float* lower, const float* lower_diag, const float* upper,
                         const float* upper_diag, int c, const float* gW, int ldw, int col_offset,
                         const float* g_logdet, float* g_lower, float* g_upper, float* g_upper_diag,
                         radmmm_stream_t stream);

/* Masked InstanceNorm1d (+ ReLU) on channels-last rows (next-row f1, the text encoder's
 * nn.InstanceNorm1d(affine=True) applied per utterance, common.py:439-441,476-484): statistics over the
 * frames t < lens[b] of item b (biased variance, eps as torch), zeros at frames >= lens[b].
 * x, y, gy, gx [B*T][ld]; mean, rstd [B][C]; dw_part, db_part [B][C] (sum over B = parameter gradients). */
int radmmm_instnorm_fwd(const float* x, int ldx, const float* weight, const float* bias, float* y, int ldy, float* mean,
                        float* rstd, const int32_t* lens, int B, int T, int C, float eps, int relu, radmmm_stream_t stream);
int radmmm_instnorm_bwd(const float* gy, int ldg, const float* x, int ldx, const float* y, int ldy, const float* weight,
                        const float* mean, const float* rstd, float* gx, int ldgx, float* dw_part, float* db_part,
                        const int32_t* lens, int B, int T, int C, int relu, radmmm_stream_t stream);

/* On-device data path (next-row f4): what the reference's CPU dataset workers compute per utterance.
 * radmmm_betabinom_prior: data.py:90-102 (beta_binomial_prior_distribution) -> out [M][P] float64, row i the pmf
 *   of BetaBinomial(P-1, scaling*(i+1), scaling*(M-i)).
 * radmmm_prior_zoom_batch: BetaBinomialInterpolator.__call__ (data.py:76-88: scipy.ndimage.zoom order=1 of the
 *   anchor prior at the rounded sizes, rows renormalised) for a whole batch, zero-padded as DataCollate does
 *   (data.py:678-679,737-741).  items: DEVICE array [B][5] of int64 {anchor pointer (float64 [bh][bw]), bh, bw,
 *   n_frames, n_tokens}; out [B][Tmax][Nmax] fp32, fully written.
 * radmmm_energy_average: data.py:363-366 (+ :339-342 when scaled): mel [B][n_mel][T] -> out [B][T]. */
int radmmm_betabinom_prior(int P, int M, double scaling, double* out, radmmm_stream_t stream);
int radmmm_prior_zoom_batch(const int64_t* items, int B, float* out, int Tmax, int Nmax, radmmm_stream_t stream);
int radmmm_energy_average(const float* mel, float* out, int B, int n_mel, int T, int scaled, radmmm_stream_t stream);

/* Optimizer step on flat fp32 buffers (next-row f3): the reference's vendored RAdam (radam.py:63-142)
 * with the global-norm clip of configs/RADMMM_train_config.yaml:7-8 folded in as a device scalar.
 * step_size / use_denom (N_sma >= 5) come from the host's step count as radam.py:101-123. */
int64_t radmmm_sumsq_scratch_floats(void);
int radmmm_sumsq(const float* x, int64_t n, float* partial, radmmm_stream_t stream);
int radmmm_radam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* clip_coef, float beta1,
                      float beta2, float eps, float step_size, float wd_lr, int use_denom, radmmm_stream_t stream);

/* torch.optim.Adam (decoupled = 0) / AdamW (decoupled = 1) on a flat fp32 buffer, with torch's arithmetic:
 *   g *= clip_coef[0] (optional device scalar);  decoupled ? p *= 1 - lr * wd : g += wd * p;
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 * The step count t lives on the device (int32 [1]): radmmm_adam_advance adds 1 to it once per optimizer step, then every
 * bucket's radmmm_adam_step reads it and derives b1^t, b2^t in double.  skip: optional device int32 [1]; when non-zero
 * neither call writes anything (p, m, v and the counter keep their bits, whatever g holds), without a host read.
 * Pointers must be 16-byte aligned; -1 before any HIP call otherwise, on a null pointer and on n <= 0. */
int radmmm_adam_advance(int32_t* step, const int32_t* skip, radmmm_stream_t stream);
int radmmm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* clip_coef, const int32_t* step,
                     const int32_t* skip, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int decoupled, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * HiFi-GAN vocoder and STFT denoiser (vocoders/hifigan_models.py:104-247, vocoders/hifigan_denoiser.py:25-58,
 * audio_processing.py:195-291).  Every convolution is a radmmm_rowgemm_f32 launch (conv_pre and the resblock convs
 * with taps/dil; ConvTranspose1d(k, u, p) as ONE row GEMM with N = u*Cout over a packed polyphase weight; the inverse
 * STFT's overlap-add the same way).  These entry points are what surrounds them.  `lens` / `frames` are int32 device
 * arrays [B] (NULL: all rows valid); rows at or past an item's length are written as 0.
 *   voc_lrelu        y[r, c] = leaky_relu(x[r, c] / div, slope), c < cols (0 in cols <= c < ldy), rows = B*T
 *   voc_conv_post    out[r] = tanh(bias[0] + sum_tap sum_c leaky_relu(x[r + tap - taps/2, c] / div, slope) *
 *                    w[tap*ldw + c]) with the shifted row inside the item (taps odd, taps*ldw <= 4096)
 *   voc_reflect_pad  xpad[b*pitch + p] = audio[b*lda + reflect(p - pad)] inside [0, lens[b]) for p < lens[b] + 2 pad,
 *                    0 beyond (caller guarantees lens[b] > pad)
 *   voc_spec_bins    spec rows [re 0..cutoff | im cutoff..2 cutoff]: mag' = max(|bin| - bias[c]*strength, 0); bin *=
 *                    mag'/|bin| (|bin| == 0: (mag', 0)).  mag_out != NULL: mag_out[r*cutoff + c] = |bin| only
 *   voc_istft_finish y [B][pitch] (overlap-add already trimmed by n_fft/2): sample n < (frames[b]-1)*hop is divided by
 *                    the window sum-square envelope of frames[b] frames at n + n_fft/2 where it exceeds FLT_MIN
 *                    (winsq: fp64 [n_fft] squared window), times n_fft/hop; 0 beyond
 *   voc_normalize    audio[b, 0:lens[b]] /= max |audio[b, 0:lens[b]]|
 * ------------------------------------------------------------------------------------ */
int radmmm_voc_lrelu(const float* x, int ldx, float* y, int ldy, int rows, int cols, int T, const int32_t* lens,
                     float div, float slope, radmmm_stream_t stream);
int radmmm_voc_conv_post(const float* x, int ldx, const float* w, int ldw, const float* bias, float* out, int rows,
                         int C, int taps, int T, const int32_t* lens, float div, float slope, radmmm_stream_t stream);
int radmmm_voc_reflect_pad(const float* audio, int lda, const int32_t* lens, float* xpad, int B, int S, int pad,
                           int pitch, radmmm_stream_t stream);
int radmmm_voc_spec_bins(float* spec, int lds, int rows, int cutoff, const float* bias, float strength, float* mag_out,
                         radmmm_stream_t stream);
int radmmm_voc_istft_finish(float* y, int B, int pitch, const int32_t* frames, const double* winsq, int n_fft, int hop,
                            radmmm_stream_t stream);
int radmmm_voc_normalize(float* audio, int lda, const int32_t* lens, int B, int S, radmmm_stream_t stream);

/* The generator's backward pass (additive entry points of ABI 4): what the row GEMMs (b_layout 1, sign -1),
 * radmmm_wgrad_f32 and radmmm_colsum do not cover.  Both run at the audio rate, one float4 per access, no atomics.
 *   voc_lrelu_bwd      the derivative factor of y = leaky_relu(x / div, slope) from the saved OUTPUT a = y (a > 0 exactly
 *                      where x > 0, div > 0).  For a row inside its item's length and c < cols (cols % 4 == 0), in this
 *                      order of exact fp32 operations:
 *                          m = a[r*lda + c] > 0 ? gy[r*ldgy + c] : gy[r*ldgy + c] * slope      (one multiply or none)
 *                          q = m / div                                                         (one division)
 *                          gx[r*ldgx + c] = accum ? gx[r*ldgx + c] + q : q                     (one addition or none)
 *                      and gx = 0 in rows at or past the length, where neither gy, a nor gx is read.  Columns cols <= c <
 *                      ld* are neither read nor written.  gx may be gy (in place).
 *   voc_conv_post_bwd  backward of voc_conv_post from its output audio = tanh(pre) and the gradient g of the audio:
 *                          dpre[r]  = g[r] * (1 - audio[r]^2) inside the length, 0 beyond (g, audio not read there)
 *                          dx[r, c] = (x[r, c] > 0 ? s : s * slope) / div,  s = sum_tap w[tap*ldw + c] * dpre[r - (tap - taps/2)]
 *                                     over the shifted rows inside the item; 0 in rows at or past the length (x not read)
 *                          dw[tap*ldw + c] = sum_r dpre[r] * leaky_relu(x[r + tap - taps/2, c] / div, slope)   (0 for c >= C)
 *                          dbias[0] = sum_r dpre[r]
 *                      dw / dbias: every workgroup adds its rows in a fixed order and leaves one partial row in scratch
 *                      (radmmm_voc_conv_post_bwd_scratch_floats(rows, C, taps, ldw) floats); a second kernel adds the
 *                      partial rows in workgroup order.  C % 4 == 0, C <= 1024, taps odd and <= 7, lddx % 4 == 0.
 * Both return the usual status as int32_t (the same type as int here): tests/test_vocoder_cpu.py pins the set of
 * `int radmmm_voc_*` declarations to the six inference entry points above. */
int32_t radmmm_voc_lrelu_bwd(const float* gy, int ldgy, const float* a, int lda, float* gx, int ldgx, int rows, int cols,
                         int T, const int32_t* lens, float div, float slope, int accum, radmmm_stream_t stream);
int64_t radmmm_voc_conv_post_bwd_scratch_floats(int rows, int C, int taps, int ldw);
int32_t radmmm_voc_conv_post_bwd(const float* x, int ldx, const float* w, int ldw, const float* audio, const float* g,
                             float* dx, int lddx, float* dw, float* dbias, float* scratch, int rows, int C, int taps,
                             int T, const int32_t* lens, float div, float slope, radmmm_stream_t stream);

/* HiFi-GAN vocoding in f16 (additive entry points of ABI 4; csrc/vocoder_f16.hip): ONE dilated Conv1d(C, C, taps,
 * dilation dil, padding "same") of a resblock on the f16 matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate), the
 * leaky-relu of its operand applied while the input tile is loaded, bias, residual and mask in the epilogue.  Rows are
 * channels-last, r = b*T + t:
 *     a(b, t, c) = h(lrelu(in_scale * X[r*ldx + c]))         for 0 <= t < lens[b], else 0
 *                  lrelu(v) = v >= 0 ? v : in_slope * v        (fp32; in_slope = 1: none)
 *                  h = round to nearest even to fp16 after the clamp to +-60000
 *     v(b, t, n) = acc_scale * sum_{tap, c} Wh[(tap*C + n)*ldw + c] * a(b, t + (tap - taps/2)*dil, c)   (fp32 accumulate)
 *     v += bias[n];  if (add) v += add[r*ldadd + n]            (in this order, fp32)
 *     Y [r*ldy  + n] = t < lens[b] ? v : 0
 *     Y2[r*ldy2 + n] = (y2_accum ? Y2[r*ldy2 + n] + : ) (t < lens[b] ? v : 0)         (Y2 optional)
 * Wh: fp16 [taps][C][ldw] holding fp16(W * s), acc_scale = 1 / s.  lens == NULL: full length.  Nothing at or past a length
 * is read into the result (X and add may hold NaN there).  Y must alias neither X, add nor Y2.  No atomics: two launches
 * give the same bits.  X and Wh 16-byte aligned, ldx % 4 == 0, ldw % 8 == 0; columns C <= c < ld* are neither read nor
 * written.
 * Shapes taken: C a multiple of 16 in 16 .. 256, taps odd and <= 11, reach (taps/2)*dil <= 40.  radmmm_voc_conv_f16_plan
 * (host only: no HIP call, no pointer dereferenced) returns RADMMM_VOC_F16_KERNEL_CODE(ntc, mi) of the instantiation a
 * descriptor reaches -- ntc column tiles of 32 and mi row tiles of 32 per wave, a workgroup owning 128 * mi frames of one
 * item -- or 0 with the reason in radmmm_last_error() for a shape that is not taken, or -1 for bad arguments (null
 * pointers, dims, pitches, alignment, aliasing).  radmmm_voc_conv_f16 returns -1 in both cases before any HIP call: no
 * kernel runs on a shape the plan refuses.  radmmm_voc_conv_f16_last_kernel: the code of the calling thread's last launch
 * (0: none yet).  (int32_t, the same type as int here, as for the two entry points above.) */
typedef struct {
  const float* X; int ldx;
  const void* Wh; int ldw;
  float* Y; int ldy;
  int B, T, C, taps, dil;
  const int32_t* lens;
  const float* bias;
  const float* add; int ldadd;
  float* Y2; int ldy2; int y2_accum;
  float in_scale, in_slope, acc_scale;
} radmmm_voc_conv_f16_desc;
#define RADMMM_VOC_F16_KERNEL_CODE(ntc, mi) ((ntc) * 100 + (mi))
int32_t radmmm_voc_conv_f16(const radmmm_voc_conv_f16_desc* d, radmmm_stream_t stream);
int32_t radmmm_voc_conv_f16_plan(const radmmm_voc_conv_f16_desc* d);
int32_t radmmm_voc_conv_f16_last_kernel(void);

/* ------------------------------------------------------------------------------------
 * WaveGlow inference (vocoders/waveglow_for_LIMMITS23/glow.py:105-175 WN.forward, :251-293 WaveGlow.infer).  The wide
 * convolutions are radmmm_rowgemm_f32 launches (the ConvTranspose1d(n_mel, n_mel, 1024, 256) upsample as ONE polyphase
 * row GEMM, cond_layer once per flow for all layers, the 3-tap dilated in_layers with taps/dil, the 1x1 res_skip
 * layers).  These entry points are what surrounds them.  Rows are GROUP steps: row r = b*Tg + g holds samples
 * g*n_group .. g*n_group + n_group - 1 of item b, Tg = T*hop/n_group.  `lens` are int32 device arrays [B] of valid
 * group steps (NULL: all rows valid); rows at or past an item's length are written as 0.  The flow variable X keeps its
 * c live channels in columns [col0, col0 + c) of an [rows][ldx] array, col0 = n_group - c, so an early re-attachment
 * writes the n_early_size columns in front of them and the final X is the waveform.  Additive entry points of ABI 4.
 *   wg_group_cond    rows[(b*Tg + g)*ldr + m*n_group + j] = up[b*up_item_stride + (g*n_group + j)*n_mel + m] (glow.py:257-258:
 *                    unfold + permute, channel order mel*n_group + j), 0 in columns n_mel*n_group .. ldr.  up is the
 *                    channels-last upsampled mel; up_item_stride >= Tg*n_group*n_mel floats (the samples a longer
 *                    transposed-convolution tail would hold past Tg*n_group are never read: the reference's trim)
 *   wg_noise_rows    X[(b*Tg + g)*ldx + col0 + c] = sigma * z[(b*ch + c)*Tg + g], z in the reference's [B][ch][Tg] layout:
 *                    the initial sigma * z and cat(sigma * z, audio) of an early re-attachment (glow.py:269, 290)
 *   wg_start         H[r, c] = bias[c] + sum_{i < n_half} W[c*n_half + i] * X[r*ldx + col0 + i]  (WN.start, n_half <= 8)
 *   wg_gate          y[r, c] = tanh(a[r, c] + cond[r, cond_off + c]) * sigmoid(a[r, C + c] + cond[r, cond_off + C + c]),
 *                    c < C: fused_add_tanh_sigmoid_multiply on layer i's slice cond_off = 2*C*i of the conditioning, in place
 *   wg_res_skip      last == 0: H[r, c] += rs[r, c], S[r, c] = (first ? 0 : S[r, c]) + rs[r, C + c];
 *                    last != 0: S[r, c] = (first ? 0 : S[r, c]) + rs[r, c] (rs has C columns, H is not touched)
 *   wg_end_coupling  o = Wend S[r] + bend (Wend [2 n_half][C]); z = [X0, (X1 - o[:n_half]) * exp(-o[n_half:])] with
 *                    X0 / X1 the two halves of X[r, col0 : col0 + 2 n_half]; X[r, col0 + i] = sum_j Winv[i*2 n_half + j]
 *                    * z[j] (the inverse 1x1 mix, Winv inverted by the caller), in place.  n_half <= 4,
 *                    2 n_half * (C + 2 n_half + 1) <= 8192
 *   wg_ungroup       audio[b*lda + g*n_group + j] = X[(b*Tg + g)*ldx + col0 + j], 0 for g >= lens[b]
 * C, lda, ldcond, cond_off, ldy, ldrs, ldh, lds % 4 == 0 and 16-byte aligned a / cond / y / rs / H / S / Wend.
 * ------------------------------------------------------------------------------------ */
int radmmm_wg_group_cond(const float* up, int64_t up_item_stride, float* rows, int ldr, const int32_t* lens, int B, int Tg,
                         int n_mel, int n_group, radmmm_stream_t stream);
int radmmm_wg_noise_rows(const float* z, float sigma, float* X, int ldx, int col0, int ch, const int32_t* lens, int B,
                         int Tg, radmmm_stream_t stream);
int radmmm_wg_start(const float* X, int ldx, int col0, int n_half, const float* W, const float* bias, float* H, int ldh,
                    int C, const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_gate(const float* a, int lda, const float* cond, int ldcond, int cond_off, float* y, int ldy, int C,
                   const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_res_skip(const float* rs, int ldrs, float* H, int ldh, float* S, int lds, int C, int first, int last,
                       const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_end_coupling(const float* S, int lds, const float* Wend, const float* bend, const float* Winv, float* X,
                           int ldx, int col0, int n_half, int C, const int32_t* lens, int rows, int T,
                           radmmm_stream_t stream);
int radmmm_wg_ungroup(const float* X, int ldx, int col0, int n_group, float* audio, int64_t lda, const int32_t* lens,
                      int B, int Tg, radmmm_stream_t stream);

/* The 16-bit GEMM modes of WaveGlow.infer ("h3": three f16 products, "f16": one): cond_layer, the in_layers and the
 * res_skip layers run on radmmm_rowgemm_h3, and these three write that GEMM's A operand -- the RADMMM_SPLIT_F16 pair of
 * the value with scale 1, [rows][ldp] halves, bit-identical to radmmm_split_f16 of the fp32 value -- in the pass that
 * computes the value.  The fp32 outputs are bit-identical to the twin's.  Rows at or past an item's length and the padding
 * columns C .. ldp are zeros in both halves; nothing is read in those rows.  C % 8 == 0, ldp % 8 == 0, ldp >= C, 16-byte
 * aligned pair arrays; the lo array may be NULL (it is not written then: the one-product GEMM takes the hi array for both
 * pointers).  Everything else as the twin.  Additive entry points of ABI 4.
 *   wg_start_split     wg_start: H fp32 and its pair Hh / Hl
 *   wg_gate_split      wg_gate: the pair yh / yl only (no fp32 copy of the gated activations exists in these modes)
 *   wg_res_skip_split  wg_res_skip: H (updated in place) and S fp32, and the updated H's pair; with last != 0 only S is
 *                      written (H, Hh, Hl may be NULL) */
int radmmm_wg_start_split(const float* X, int ldx, int col0, int n_half, const float* W, const float* bias, float* H,
                          int ldh, void* Hh, void* Hl, int ldp, int C, const int32_t* lens, int rows, int T,
                          radmmm_stream_t stream);
int radmmm_wg_gate_split(const float* a, int lda, const float* cond, int ldcond, int cond_off, void* yh, void* yl, int ldp,
                         int C, const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_res_skip_split(const float* rs, int ldrs, float* H, int ldh, float* S, int lds, void* Hh, void* Hl, int ldp,
                             int C, int first, int last, const int32_t* lens, int rows, int T, radmmm_stream_t stream);

/* The other direction of the same flow (glow.py:207-249 WaveGlow.forward: audio -> latent z and the terms of its
 * likelihood), same conventions; the WN between the mix and the coupling is the launch sequence of the inverse
 * direction (wg_start reads the mixed values).  Additive entry points of ABI 4.
 *   wg_group_audio       X[(b*Tg + g)*ldx + j] = audio[b*lda + g*n_group + j], j < n_group, 0 for g >= lens[b] (the inverse
 *                        of wg_ungroup; samples past an item's length are never read, so a NaN there cannot reach X)
 *   wg_mix_fwd           X[r, col0 + i] = sum_j W[i*c + j] * X[r, col0 + j] in place, W = convinv.conv.weight itself,
 *                        c even, 2 <= c <= 8
 *   wg_end_coupling_fwd  o = Wend S[r] + bend; b = o[:n_half], log_s = o[n_half:]; X1 = exp(log_s) * X1 + b in place (X1 the
 *                        second half of X[r, col0 : col0 + 2 n_half], the first half is not touched);
 *                        ls[r] = (first ? 0 : ls[r]) + sum_i log_s[i]; log_s != NULL: log_s[r*n_half + i] = log_s[i].
 *                        The limits of wg_end_coupling: n_half <= 4, 2 n_half * (C + 2 n_half + 1) <= 8192
 *   wg_nll_parts         parts[b][0] = sum of X[r, j]^2 over the valid rows of item b and j < n_group, parts[b][1] = sum
 *                        of ls[r] over the same rows; float64 sums in a fixed order, one workgroup per item, no
 *                        atomics: bitwise repeatable, and an item's sums do not depend on the rest of the batch */
int radmmm_wg_group_audio(const float* audio, int64_t lda, float* X, int ldx, int n_group, const int32_t* lens, int B,
                          int Tg, radmmm_stream_t stream);
int radmmm_wg_mix_fwd(float* X, int ldx, int col0, int c, const float* W, const int32_t* lens, int rows, int T,
                      radmmm_stream_t stream);
int radmmm_wg_end_coupling_fwd(const float* S, int lds, const float* Wend, const float* bend, float* X, int ldx, int col0,
                               int n_half, int C, float* ls, int first, float* log_s, const int32_t* lens, int rows,
                               int T, radmmm_stream_t stream);
int radmmm_wg_nll_parts(const float* X, int ldx, int n_group, const float* ls, const int32_t* lens, int B, int Tg,
                        double* parts, radmmm_stream_t stream);

/* The backward pass of that direction: what the row GEMMs (b_layout 1), radmmm_wgrad_f32 and radmmm_colsum do not cover.
 * Rows at or past an item's length are never read, and every gradient row there is written as 0.  No atomics: every
 * result is bitwise repeatable.  Additive entry points of ABI 4.
 *   wg_coupling_bwd  o = Wend S[r] + bend recomputed as wg_end_coupling_fwd does; x1 = Xs[r, col0 + n_half ..] the
 *                    coupling's saved input, g = dX[r, col0 + n_half ..] the gradient of its output:
 *                      dO[r] = [g, g * exp(log_s) * x1 + g_ls]  ([rows][2 n_half]: the gradient of o)
 *                      dX[r, col0 + n_half + k] = g[k] * exp(log_s[k])  in place
 *                      dS[r, :] = Wend^T dO[r]
 *                    g_ls: ldg == 0: one device value for every row and channel (the likelihood's -1/N); else
 *                    g_ls[r*ldg + k].  The limits of wg_end_coupling.
 *   wg_gate_bwd      dA[r, c] = g[r, c] * sig * (1 - tanh^2), dA[r, C + c] = g[r, c] * tanh * sig * (1 - sig), tanh and
 *                    sig of wg_gate's arguments a[r, :] + cond[r, cond_off:]; dA may be a column slice of the
 *                    conditioning gradient (ldda its pitch)
 *   wg_start_bwd     dX[r, col0 + i] += sum_c Wt[i*C + c] * dH[r, c], Wt [n_half][C] the start weight transposed, n_half <= 4
 *   wg_outer_reduce  out[m*N + n] = sum over the valid rows of A[r*lda + m] * B[r*ldb + n], m < M <= 8 (A == NULL: M = 1,
 *                    A = 1: column sums): the weight / bias gradients of end, start and the 1x1 mix.  One partial per
 *                    256-row tile in scratch (radmmm_wg_outer_reduce_scratch_floats(rows, M, N) floats), added in tile
 *                    order by radmmm_colsum_final.
 *   wg_inv_logdet    for n <= 32 square matrices of sizes cs[k] <= 8 (a HOST array) packed one after the other in W:
 *                    Winv (same packing, fp32) and logdet[k] = log|det W_k| (float64) by Gauss-Jordan elimination with
 *                    partial pivoting in float64, one launch: the training step never leaves the device for them
 *   wg_ungroup_cond  the inverse permutation of wg_group_cond: up[b*up_item_stride + (g*n_group + j)*n_mel + m] =
 *                    rows[(b*Tg + g)*ldr + m*n_group + j], 0 for g >= lens[b] */
int radmmm_wg_coupling_bwd(const float* S, int lds, const float* Wend, const float* bend, const float* Xs, int ldxs,
                           float* dX, int ldx, int col0, int n_half, int C, const float* g_ls, int ldg, float* dO,
                           float* dS, int ldds, const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_gate_bwd(const float* a, int lda, const float* cond, int ldcond, int cond_off, const float* g, int ldg,
                       float* dA, int ldda, int C, const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_start_bwd(const float* dH, int ldh, const float* Wt, float* dX, int ldx, int col0, int n_half, int C,
                        const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_outer_reduce(const float* A, int lda, int M, const float* B, int ldb, int N, float* out, float* scratch,
                           const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int64_t radmmm_wg_outer_reduce_scratch_floats(int rows, int M, int N);
int radmmm_wg_inv_logdet(const float* W, const int32_t* cs, int n, float* Winv, double* logdet, radmmm_stream_t stream);
int radmmm_wg_ungroup_cond(const float* rows, int ldr, float* up, int64_t up_item_stride, const int32_t* lens, int B,
                           int Tg, int n_mel, int n_group, radmmm_stream_t stream);

/* Training on the f16 matrix cores (WaveGlow.train_precision "h3"): the two gradient producers of that backward pass also
 * write, in the pass that computes the value, the RADMMM_SPLIT_F16 pair of scale * value -- the A operand of the data
 * gradient (radmmm_rowgemm_h3) and the GY operand of the weight gradient (radmmm_wgrad_rm).  The conventions of the
 * forward *_split kernels: [rows][ldp] halves, 8 columns per thread and one 16-byte store per half array; the pair is
 * bit-identical to radmmm_split_f16(the fp32 output, scale); the fp32 outputs are bit-identical to the twin's; rows at or
 * past an item's length are zeros in both halves and nothing is read there.  A row of the pair is `pcols` columns wide:
 * the values, then zeros up to pcols (pcols == the value count: nothing else is written, so the pair may be a column
 * slice of a wider [rows][ldp] buffer, as the fp32 output may).  C, ldp, pcols % 8 == 0, pcols <= ldp, 16-byte aligned
 * pair arrays.  scale: a power of two (the gradient scale); sat_flag: optional device int, OR-ed with bit 0 when
 * |scale * value| > 60000 was clamped (radmmm_split_opts.sat_flag): the only atomic, every result is bitwise repeatable.
 * Everything else as the twin.  Additive entry points of ABI 4.
 *   wg_coupling_bwd_split  wg_coupling_bwd + the pair dSh / dSl of scale * dS (C values per row, C <= pcols)
 *   wg_gate_bwd_split      wg_gate_bwd + the pair dAh / dAl of scale * dA (2 C values per row, 2 C <= pcols) */
int radmmm_wg_coupling_bwd_split(const float* S, int lds, const float* Wend, const float* bend, const float* Xs, int ldxs,
                                 float* dX, int ldx, int col0, int n_half, int C, const float* g_ls, int ldg, float* dO,
                                 float* dS, int ldds, void* dSh, void* dSl, int ldp, int pcols, float scale,
                                 int32_t* sat_flag, const int32_t* lens, int rows, int T, radmmm_stream_t stream);
int radmmm_wg_gate_bwd_split(const float* a, int lda, const float* cond, int ldcond, int cond_off, const float* g, int ldg,
                             float* dA, int ldda, void* dAh, void* dAl, int ldp, int pcols, int C, float scale,
                             int32_t* sat_flag, const int32_t* lens, int rows, int T, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Batched synthesis glue (TTSModel.sample_full / reconstruct_from_batch_attributes, tts_lightning_modules.py:286-437).
 * Additive entry points of ABI 4.  No floating-point atomics: every result is bitwise repeatable.
 *   synth_durations  per token t of utterance b (x[b*item_stride + t], fp32): d = min(max(rint(x), 1), 65536) for
 *                    t < text_lens[b], else 0 (rint rounds half to even, as torch.round).  integer_mode != 0: d =
 *                    min(max(x, 0), 65536) truncated, no rounding and no clamp to 1 (durations that are integers already).
 *                    The cap of 65536 frames per token guards against non-finite or absurd predictions (NaN -> the lower
 *                    bound); the reference has none.  Writes dur [B][Tt] and its inclusive prefix sum cum [B][Tt] (int32)
 *                    and out_lens[b] = sum_t dur.  text_lens NULL: every token valid.  Tt <= 32767.
 *   synth_regulate   LengthRegulator (common.py:208-237) into channels-last frame rows: rows[(b*Tmax + t)*ldc + c] =
 *                    txt[b*item_stride + j*row_stride + c] for t < out_lens[b], c < C, j the token whose prefix-sum range
 *                    holds t; zeros elsewhere (frames past out_lens[b], channels C..ldc).  A pure copy.  C, ldc,
 *                    row_stride, item_stride % 4 == 0, 16-byte aligned txt / rows, Tt <= 16384.
 *   synth_f0_stats   partials[k*nparts + i], k = count / sum / sum of squares (fp64) of f0 over the frames t < lens[b]
 *                    with sigmoid(voiced_logit) > 0.5, workgroup i of nparts (1..1024)
 *   synth_f0_apply   contiguous [B][T] outputs: voiced_out = (t < lens[b] && sigmoid(voiced_logit) > 0.5); f0_out = f0 *
 *                    voiced, and with partials (from synth_f0_stats) (f0 - mu) / sigma * f0_std[b] + f0_mean[b] on the
 *                    voiced frames (pooled mean and unbiased std of the whole batch, tts_lightning_modules.py:367-376),
 *                    left unshifted when fewer than 2 voiced frames exist or sigma == 0; energy_out = energy masked to
 *                    lens[b]
 * ------------------------------------------------------------------------------------ */
int radmmm_synth_durations(const float* x, int64_t item_stride, const int32_t* text_lens, int B, int Tt, int integer_mode,
                           int32_t* dur, int32_t* cum, int32_t* out_lens, radmmm_stream_t stream);
int radmmm_synth_regulate(const float* txt, int64_t item_stride, int row_stride, int Tt, int C, const int32_t* cum,
                          const int32_t* out_lens, int B, int Tmax, float* rows, int ldc, radmmm_stream_t stream);
int radmmm_synth_f0_stats(const float* f0, int64_t f0_stride, const float* voiced_logit, int64_t v_stride,
                          const int32_t* lens, int B, int T, double* partials, int nparts, radmmm_stream_t stream);
int radmmm_synth_f0_apply(const float* f0, int64_t f0_stride, const float* voiced_logit, int64_t v_stride,
                          const float* energy, int64_t e_stride, const int32_t* lens, int B, int T, const double* partials,
                          int nparts, const float* f0_mean, const float* f0_std, float* f0_out, float* energy_out,
                          float* voiced_out, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training batches built on the device (data.py:419-610 AudioDataset.__getitem__ after the file reads, :616-790
 * DataCollate): ragged utterances packed back to back in one staging buffer -> the padded tensors of a batch.
 * offsets are int64 DEVICE arrays [B] in elements of the packed array, lens / frames / in_lens int32 device arrays [B].
 *   collate_scratch_floats  size of `scratch` (the layout of radmmm_stft_mel at S = Smax; the reflect-padded rows
 *                    xpad [B][pitch], pitch = roundup4(Smax + n_fft), sit at its start)
 *   collate_unpack_pad  xpad[b][p] = src[offsets[b] + reflect(p - n_fft/2)] * scale inside [0, lens[b]) for
 *                    p < lens[b] + n_fft, 0 beyond.  src: int16 (src_int16 != 0) or fp32 samples.  audio != NULL:
 *                    audio[b][j] = src[offsets[b] + j] * scale for j < lens[b], 0 for lens[b] <= j < Smax, in the same
 *                    pass.  Caller guarantees n_fft/2 < lens[b] <= Smax.  Offsets that are multiples of 4 let the
 *                    interior go through 8 / 16-byte loads.
 *   collate_mel      the two row GEMMs of radmmm_stft_mel over B*Tmax rows (Tmax = 1 + Smax/hop) of the xpad that
 *                    collate_unpack_pad left in `scratch`, then mel[b][c][t] = log(max(., clip)) for t < frames[b], 0
 *                    beyond, and (energy != NULL) energy[b][t] = mean_c mel[b][c][t], (x + 20) / 20 when scaled, 0 beyond
 *                    -- the sums in the order of radmmm_energy_average.  mel [B][n_mel][Tmax], energy [B][Tmax].
 *   collate_tracks   one workgroup per utterance: f0[b][t] = f0_normalize(f0_packed[frame_offsets[b] + t])
 *                    (use_log_f0: x >= f0_min ? log(x) : 0, data.py:321-327) and, with distance_tx, minus max(log d, 0),
 *                    d the distance in frames to the nearest frame of the utterance with f0 > 0 (data.py:527-532: the 1-D
 *                    scipy.ndimage.distance_transform_edt(f0 <= 0); without any such frame d = t + 1, as scipy returns); log
 *                    and subtraction in double, rounded once.  p_voiced / voiced_mask copied; all three zero for frames[b]
 *                    <= t < Tmax.  text[b][l] = ids_packed[token_offsets[b] + l] for l < in_lens[b], else 0 (int64
 *                    [B][Lmax]).  meta_dst[0..n_meta) = meta_src[0..n_meta) (8-byte words: the per-item scalars of the
 *                    batch).  Any of the three tracks, text and meta may be NULL / 0.  scan: int32 [B][Tmax] scratch,
 *                    needed with f0 and distance_tx.  No cap on Tmax.
 * ------------------------------------------------------------------------------------ */
int64_t radmmm_collate_scratch_floats(int B, int Smax, int n_fft, int hop, int n_mel);
int radmmm_collate_unpack_pad(const void* src, int src_int16, const int64_t* offsets, const int32_t* lens,
                              float* scratch, float* audio, int B, int Smax, int n_fft, float scale,
                              radmmm_stream_t stream);
int radmmm_collate_mel(const float* basis, const float* mel_basis, const int32_t* frames, float* mel, float* energy,
                       float* scratch, int B, int Smax, int n_fft, int hop, int n_mel, float clip, int scaled,
                       radmmm_stream_t stream);
int radmmm_collate_tracks(const float* f0_packed, const float* p_voiced_packed, const float* voiced_mask_packed,
                          const int32_t* ids_packed, const int64_t* frame_offsets, const int64_t* token_offsets,
                          const int32_t* frames, const int32_t* in_lens, float* f0, float* p_voiced, float* voiced_mask,
                          int64_t* text, int32_t* scan, const int64_t* meta_src, int64_t* meta_dst, int n_meta, int B,
                          int Tmax, int Lmax, float f0_min, int use_log_f0, int distance_tx, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Multi-resolution STFT loss (stft_loss.py: STFTLoss.forward, SpectralConvergenceLoss, LogSTFTMagnitudeLoss,
 * AWeightedLogSTFTMagnitudeLoss with its weights of 1.0), forward and backward (additive entry points of ABI 4).  The
 * DFT and its data gradient are radmmm_rowgemm_f32 launches (frames x basis, dspec x basis with b_layout 1); these
 * entry points are what surrounds them.  One resolution: n_fft (even), hop >= 1, win <= n_fft, T samples per item with
 * T > n_fft/2 (torch.stft's reflect pad of h = n_fft/2 at the padded length T), F = 1 + T/hop frames per item, the
 * window at columns [left, left + win) of a frame, left = (n_fft - win)/2, cutoff = n_fft/2 + 1 bins.  `frames` is an
 * int32 device array [B] of valid frames per item, read clamped to [0, F] everywhere, also in the sum S of stftloss_finish
 * (the reference's semantics for len_ratios in [0, 1]; its lens.sum() would keep a count above F); NULL: every frame is valid AND the
 * reference's lens=None forms apply (finish / bwd).  Rows are r = b*F + f.  No atomics, fixed reduction orders.
 *   stftloss_frame    A[r*ldk + j] = x[b*ldx + reflect(f*hop + left + j - h)] for j < win and f < frames[b], reflected
 *                     about 0 and about T-1; 0 for win <= j < ldk and in rows f >= frames[b] (x not read there).
 *                     ldk % 4 == 0, ldk >= win, A 16B aligned, B*F*ldk*4 < 2 GiB.
 *   stftloss_terms    spec_* [B*F][lds], re in columns [0, cutoff), im in [cutoff, 2 cutoff) (lds % 4 == 0; columns past
 *                     2 cutoff are not read): mag = sqrt(max(re^2 + im^2, 1e-7)); part[4r .. 4r+3] = (sum_k (ym - xm)^2,
 *                     sum_k ym^2, sum_k |log ym - log xm|, 0), with a_weighting |log(ym + 1) - log(xm + 1)|.  One wave per
 *                     row: lane l adds bins l, l+64, ... in order, then a xor butterfly.  Rows f >= frames[b]: zeros,
 *                     spec not read.
 *   stftloss_finish   one workgroup, fp64: norm = (S, sum_r D_r, sum_r N_r, 0) over the valid rows, S = sum_b frames[b]
 *                     (B*F without frames).  out[0] = sum_r sqrt(D_r)/sqrt(N_r) / S with frames, sqrt(sum D)/sqrt(sum N)
 *                     without; out[1] = sum_r L_r / (S * cutoff).
 *   stftloss_bwd      gradients of g_sc[0]*scale*out[0] + g_mag[0]*scale*out[1] (g_sc, g_mag: device scalars) with respect
 *                     to the spectra, dspec_x and / or dspec_y (either may be NULL) [B*F][lds]: per bin dmag * re/mag and
 *                     dmag * im/mag where re^2 + im^2 >= 1e-7, 0 below; sign(0) = 0 in the log term; rows (the total,
 *                     without frames) with sum (ym - xm)^2 == 0 add nothing to the spectral-convergence term.  Rows
 *                     f >= frames[b] and columns 2 cutoff <= c < lds are written as 0.
 *   stftloss_unframe  the adjoint of stftloss_frame in gather form: dx[b*lddx + s], s < T, is the sum of dA over the
 *                     frames f < frames[b] (ascending) that hold padded position s + h, then h - s for 1 <= s <= h, then
 *                     h + 2(T-1) - s for T-1-h <= s <= T-2; with accum the sum is added to dx[b*lddx + s] (last).
 * ------------------------------------------------------------------------------------ */
int radmmm_stftloss_frame(const float* x, int ldx, const int32_t* frames, float* A, int ldk, int B, int T, int F,
                          int n_fft, int hop, int win, radmmm_stream_t stream);
int radmmm_stftloss_terms(const float* spec_x, const float* spec_y, int lds, const int32_t* frames, float* part, int B,
                          int F, int cutoff, int a_weighting, radmmm_stream_t stream);
int radmmm_stftloss_finish(const float* part, const int32_t* frames, float* out, double* norm, int B, int F, int cutoff,
                           radmmm_stream_t stream);
int radmmm_stftloss_bwd(const float* spec_x, const float* spec_y, int lds, const float* part, const double* norm,
                        const int32_t* frames, const float* g_sc, const float* g_mag, float scale, float* dspec_x,
                        float* dspec_y, int B, int F, int cutoff, int a_weighting, radmmm_stream_t stream);
int radmmm_stftloss_unframe(const float* dA, int ldk, const int32_t* frames, float* dx, int lddx, int B, int T, int F,
                            int n_fft, int hop, int win, int accum, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Differentiable log-mel and the mel L1 loss (audio_processing.py: TacotronSTFT.mel_spectrogram, STFT.transform, applied to
 * each item alone, under F.l1_loss over the valid frames), forward and backward (additive entry points of ABI 4).  The
 * three dense products are radmmm_rowgemm_f32 launches (frames x forward_basis, mag x mel_basis^T; dmelp x mel_basis and
 * dspec x forward_basis with b_layout 1); these entry points are what surrounds them.  Geometry: n_fft (a multiple of 4),
 * hop >= 1, h = n_fft/2, cutoff = n_fft/2 + 1, B items of at most S samples (S > h), F = 1 + S/hop rows per item, r = b*F + f.
 * `lens` is an int32 device array [B] of samples per item, read clamped into [1, S] (NULL: S everywhere): item b is
 * reflect-padded by h about 0 and about lens[b] - 1 and has 1 + lens[b]/hop frames.  The caller keeps lens[b] > h; below
 * that every reflected index is clamped into [0, lens[b] - 1], so nothing is read or written outside an item and the
 * item's numbers are unspecified but finite.  A mel in the reference layout is [B][n_mel][Ft].  `frames` (int32 device
 * array [B] or NULL) caps the frames of an item that enter the loss: n[b] = min(1 + lens[b]/hop, Ft, frames[b] clamped into
 * [0, min(F, Ft)]).  No atomics, fixed reduction orders.
 *   melloss_frame    A[r*n_fft + j] = x[b*ldx + reflect(f*hop + j - h)] for f < 1 + lens[b]/hop; zeros in the other rows
 *                    (x not read there, nor at or past lens[b]).  A 16B aligned, B*F*n_fft*4 < 2 GiB.
 *   melloss_mag      spec [B*F][lds], re in columns [0, cutoff), im in [cutoff, 2 cutoff) -> mag[r*ldm + k] =
 *                    sqrt(re^2 + im^2) (no clamp); 0 for cutoff <= k < ldm and in rows past an item's frames (spec not read
 *                    there).  lds, ldm % 4 == 0.
 *   melloss_terms    melp [B*F][ldn] -> mel = log(max(melp, clip)), the log taken in double and rounded once (melloss_bwd
 *                    forms the same bits).  mel_out (or NULL) [B][n_mel][F]: the mel, exact zeros
 *                    past an item's frames.  target [B][n_mel][Ft] with part [B*F] (both or neither): part[r] =
 *                    sum_c |mel - target[b][c][f]| for f < n[b], else 0; lane l of the row's wave adds channels l, l+64, ...
 *                    in order, then a xor butterfly.  melp is not read in rows past an item's frames or in columns
 *                    >= n_mel, target not at frames >= n[b].
 *   melloss_finish   one workgroup, fp64: norm[0] = sum_b n[b]; out[0] = sum_{f < n[b]} part / (n_mel * norm[0]), 0 when
 *                    norm[0] == 0.
 *   melloss_bwd      dmelp [B*F][ldn].  With target (and norm, g; dmel NULL): g[0] * sign(mel - target) / (n_mel * norm[0])
 *                    / melp for f < n[b], the sign recomputed from melp and target as melloss_terms formed it, sign(0) = 0.
 *                    With dmel [B][n_mel][F] (target NULL): dmel[b][c][f] / melp for f < 1 + lens[b]/hop.  In both: 0 where
 *                    melp < clip, in every other row and in columns n_mel <= c < ldn.
 *   melloss_dspec    dspec[r] = (dmag * re/mag | dmag * im/mag) with mag recomputed from spec as melloss_mag forms it; 0
 *                    where mag == 0, in rows past an item's frames (nothing read there) and in columns 2 cutoff <= c < lds.
 *   melloss_unframe  the adjoint of melloss_frame in gather form: dx[b*lddx + s], s < lens[b], is the sum of dA [B*F][n_fft]
 *                    over the item's frames (ascending) that hold padded position s + h, then h - s for 1 <= s <= h, then
 *                    h + 2(lens[b]-1) - s for lens[b]-1-h <= s <= lens[b]-2; with accum the sum is added to dx (last).
 *                    Samples lens[b] <= s < S get 0 (left as they are with accum).
 * ------------------------------------------------------------------------------------ */
int radmmm_melloss_frame(const float* x, int ldx, const int32_t* lens, float* A, int B, int S, int F, int n_fft, int hop,
                         radmmm_stream_t stream);
int radmmm_melloss_mag(const float* spec, int lds, const int32_t* lens, float* mag, int ldm, int B, int S, int F, int hop,
                       int cutoff, radmmm_stream_t stream);
int radmmm_melloss_terms(const float* melp, int ldn, const int32_t* lens, const int32_t* frames, const float* target, int Ft,
                         float* mel_out, float* part, int B, int S, int F, int hop, int n_mel, float clip,
                         radmmm_stream_t stream);
int radmmm_melloss_finish(const float* part, const int32_t* lens, const int32_t* frames, float* out, double* norm, int B,
                          int S, int F, int Ft, int hop, int n_mel, radmmm_stream_t stream);
int radmmm_melloss_bwd(const float* melp, int ldn, const int32_t* lens, const int32_t* frames, const float* target, int Ft,
                       const double* norm, const float* g, const float* dmel, float* dmelp, int B, int S, int F, int hop,
                       int n_mel, float clip, radmmm_stream_t stream);
int radmmm_melloss_dspec(const float* dmag, int ldm, const float* spec, int lds, const int32_t* lens, float* dspec, int B,
                         int S, int F, int hop, int cutoff, radmmm_stream_t stream);
int radmmm_melloss_unframe(const float* dA, const int32_t* lens, float* dx, int lddx, int B, int S, int F, int n_fft, int hop,
                           int accum, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * HiFi-GAN multi-period discriminator (hifigan_models.py: DiscriminatorP, MultiPeriodDiscriminator) and the GAN losses of
 * loss.py (gan_feature_loss, gan_discriminator_loss, gan_generator_loss), forward and backward (additive entry points of
 * ABI 4).  Every convolution but conv_post is a radmmm_rowgemm_f32 launch in its framed form, every weight gradient a
 * radmmm_wgrad_f32 launch over an explicit frame matrix, every bias gradient a radmmm_colsum; these entry points are what
 * surrounds them.  Geometry of one discriminator of period p on B items of T samples, real and generated stacked:
 *   H = ceil(T / p) rows of the fold x[b][h][w] = audio[b][refl(h*p + w)], refl(t) = t < T ? t : 2(T-1) - t  (T > H*p - T);
 *   S = 2*B*p sequences, s = (sig*B + b)*p + w, sig 0 real, 1 generated;
 *   a conv of 5 taps, stride st, zero pad 2 maps H rows to Ho = (H-1)/st + 1 rows: out[h'] = sum_k W[k] . in[st*h' - 2 + k];
 *   a PADDED map is [S][H + 4][C] floats, rows 2 .. H + 1 the map, the other four rows zero, C % 4 == 0: the window of
 *   output row h' is the 5*C contiguous floats at padded row st*h';  a DENSE matrix is [S*H][C];  the discriminator
 *   output is [2B][H][p], real half first (the reference's flatten: position h*p + w).
 * `cnt` is an int32 device array [7][B] or NULL (everything counts): row l < 6 the rows of map l that count for item b
 * (read clamped to [0, H_l]), row 6 the positions of the flattened output that count (clamped to [0, H_5 * p]).
 * lrelu(v) = v > 0 ? v : slope * v; its derivative is taken from the saved OUTPUT y: y > 0 ? 1 : slope.
 *   mpd_fold_frame       F[(s*H1 + h')*8 + k] = x_s[3h' - 2 + k] for k < 5 and the row inside [0, H), else 0 (k = 5 .. 7 pad
 *                        the row to 8 floats).  A copy.  H1 = (H-1)/3 + 1.
 *   mpd_repad            X[s][r][c] = lrelu(Z[(s*H + r - 2)*ldz + c]) for 2 <= r < H + 2, else 0.
 *   mpd_frame            F[(s*Ho + h')*5C + j] = X[s][st*h'][j], j < 5C.  A copy.  st*(Ho-1) + 5 <= H + 4.
 *   mpd_unframe          dZ[(s*H + h)*C + c] = (sum_h' dF[(s*Ho + h')*5C + (h + 2 - st*h')*C + c] + add[s][h + 2][c]) *
 *                        lrelu'(X[s][h + 2][c]) over the windows 0 <= h' < Ho that hold row h, ascending; add (padded
 *                        layout, its pad rows never read) may be NULL.
 *   mpd_conv_post        out[(s2*H + h)*p + w] = bias[0] + sum_{k<3} sum_c X[s2*p + w][h + 1 + k][c] * W[k*C + c]  (3 taps,
 *                        zero pad 1); one wave per output, lane l adds columns 4l .. 4l+3, 4l+256 .. per tap, then a xor butterfly.
 *   mpd_conv_post_dgrad  dZ[(s*H + h)*C + c] = (sum_k dOut[s2][h + 1 - k][w] * W[k*C + c] + add[s][h + 2][c]) *
 *                        lrelu'(X[s][h + 2][c]), rows outside [0, H) skipped.
 *   mpd_conv_post_wgrad  part [mpd_conv_post_wgrad_parts][3C + 1]: per chunk of 64 rows (s, h), ascending,
 *                        part[j][k*C + c] = sum dOut[s2][h][w] * X[s][h + 1 + k][c], part[j][3C] = sum dOut;
 *                        radmmm_colsum_final(part, out, parts, 3C + 1) adds the chunks.
 *   mpd_unfold_audio     g[b*ldg + t] = G(t) + (T <= 2(T-1) - t < H*p ? G(2(T-1) - t) : 0), G(u) = sum over the windows h'
 *                        (ascending) that hold row u/p of dF[(s*H1 + h')*8 + u/p + 2 - 3h'], s = (sig*B + b)*p + u%p.
 *   mpd_fm_terms         part [mpd_fm_terms_parts] partial sums of |r - g| over the elements (b, w, h < cnt[b], c) of one map
 *                        (padded != 0: a padded map; 0: the dense output with C = 1); cnt is the map's own row [B].
 *   mpd_finish           one workgroup, fp64.  part holds the six maps' partials, map l at [off[l], off[l+1]) (off, C, H are
 *                        HOST arrays of 7, 6, 6 ints).  norm[l] = sum_b cnt[l][b] * C_l * p, norm[6] = sum_b cnt[6][b];
 *                        res = (sum_l sum(part_l) / norm[l], sum m (1-dr)^2 / norm[6], sum m dg^2 / norm[6],
 *                        sum m (1-dg)^2 / norm[6]), m = [h*p + w < cnt[6][b]].
 *   mpd_fm_grad          G (padded, pad rows not written) = +-(up[0] / norm[0]) * sign(r - g) * [h < cnt[b]], + on the real
 *                        half, sign(0) = 0; cnt and norm are the map's own.
 *   mpd_out_grad         dOut real = -2 (1-dr) m up[1] / norm[6] + f, generated = (2 dg up[2] - 2 (1-dg) up[3]) m / norm[6] - f,
 *                        f = up[0] / norm[5] * sign(dr - dg) * [h < cnt[5][b]]; up is a device array of 4 floats.
 * No atomics, fixed reduction orders.
 * ------------------------------------------------------------------------------------ */
int radmmm_mpd_fold_frame(const float* y, const float* y_hat, int ldy, float* F, int B, int T, int p, int H, int H1,
                          radmmm_stream_t stream);
int radmmm_mpd_repad(const float* Z, int ldz, float* X, int S, int H, int C, float slope, radmmm_stream_t stream);
int radmmm_mpd_frame(const float* X, float* F, int S, int H, int C, int Ho, int stride, radmmm_stream_t stream);
int radmmm_mpd_unframe(const float* dF, const float* add, const float* X, float* dZ, int S, int H, int C, int Ho, int stride,
                       float slope, radmmm_stream_t stream);
int radmmm_mpd_conv_post(const float* X, const float* W, const float* bias, float* out, int B2, int p, int H, int C,
                         radmmm_stream_t stream);
int radmmm_mpd_conv_post_dgrad(const float* dOut, const float* W, const float* add, const float* X, float* dZ, int B2, int p,
                               int H, int C, float slope, radmmm_stream_t stream);
int64_t radmmm_mpd_conv_post_wgrad_parts(int B2, int p, int H);
int radmmm_mpd_conv_post_wgrad(const float* dOut, const float* X, float* part, int B2, int p, int H, int C,
                               radmmm_stream_t stream);
int radmmm_mpd_unfold_audio(const float* dF, float* g, int ldg, int B, int T, int p, int H, int H1, int sig,
                            radmmm_stream_t stream);
int64_t radmmm_mpd_fm_terms_parts(int B, int p, int H, int C);
int radmmm_mpd_fm_terms(const float* X, const int32_t* cnt, float* part, int B, int p, int H, int C, int padded,
                        radmmm_stream_t stream);
int radmmm_mpd_finish(const float* part, const int32_t* off, const int32_t* C, const int32_t* H, const float* out,
                      const int32_t* cnt, float* res, double* norm, int B, int p, radmmm_stream_t stream);
int radmmm_mpd_fm_grad(const float* X, const int32_t* cnt, const double* norm, const float* up, float* G, int B, int p, int H,
                       int C, radmmm_stream_t stream);
int radmmm_mpd_out_grad(const float* out, const int32_t* cnt, const double* norm, const float* up, float* dOut, int B, int p,
                        int H, radmmm_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The multi-period discriminator's precision "h3" (csrc/mpd_h3.hip; additive entry points of ABI 4): the producers that feed
 * the wide convs' three passes to radmmm_rowgemm_h3 / radmmm_wgrad_rm without an fp32 round trip.  Every pair is
 * RADMMM_SPLIT_F16 of scale * value, element for element the bits of radmmm_split_f16; sat_flag (or NULL) as
 * radmmm_split_opts.sat_flag, bit 0.  C % 8 == 0, 16-byte aligned arrays, pair pitches % 8 == 0; columns of a pair row at
 * or beyond the matrix' width are left alone.  rows_pad: the pair holds max(rows, rows_pad) rows and the rows from `rows`
 * on are written as zeros (radmmm_wgrad_rm contracts at least 32 rows; zero rows add nothing).  Memory-bound passes, no
 * reductions: equal inputs give equal bits.  Bad arguments return -1 before any HIP call.
 *   radmmm_mpdh3_repad            radmmm_mpd_repad (the same fp32 map X, bit for bit) + the map's pair Xh / Xl in the same
 *                                  padded layout [S][H + 4][C], pad rows zero: the framed A operand of the next conv
 *                                  (radmmm_rowgemm_h3 with a_item_stride = (H + 4) * C, lda_h = stride * C, K = 5 * C)
 *   radmmm_mpdh3_frame            radmmm_mpd_frame written as a pair: Fh / Fl [max(S * Ho, rows_pad)][ldf], row
 *                                  (s, h') = the 5 * C values of map s from padded row stride * h' on; no fp32 frames
 *   radmmm_mpdh3_unframe          radmmm_mpd_unframe (the same dZ, bit for bit; dZ may be NULL) + the pair dZh / dZl
 *                                  [max(S * H, rows_pad)][ldh] of scale * dZ
 *   radmmm_mpdh3_conv_post_dgrad  radmmm_mpd_conv_post_dgrad in the same way
 *   radmmm_mpdh3_plan             host only, like radmmm_rowgemm_h3_plan (< 0: bad dims): 1 when the dense 5-tap conv Cin -> Cout of stride `stride` on S
 *                                  sequences of Hin rows (Hout windows) can run its three passes on the split kernels as
 *                                  the discriminator launches them -- the framed forward GEMM and the data-gradient GEMM
 *                                  pass radmmm_rowgemm_h3's plan, the weight gradient radmmm_wgrad_rm's checks at
 *                                  max(S * Hout, 32) rows and one tap -- else 0 with the reason in radmmm_last_error
 * radmmm_rowgemm_h3 takes the framed descriptor for this (ABI 4, additive): base.a_item_stride != 0, in HALVES of Ah / Al:
 * item b, frame t at b * a_item_stride + t * lda_h, rows may overlap (lda_h < K); one tap, no extra segment, a_mask_mode 0,
 * three or one product; a_item_stride % 8 == 0.
 * ------------------------------------------------------------------------------------ */
int radmmm_mpdh3_repad(const float* Z, int ldz, float* X, void* Xh, void* Xl, int S, int H, int C, float slope, float scale,
                        int32_t* sat_flag, radmmm_stream_t stream);
int radmmm_mpdh3_frame(const float* X, void* Fh, void* Fl, int ldf, int S, int H, int C, int Ho, int stride, int rows_pad,
                        float scale, int32_t* sat_flag, radmmm_stream_t stream);
int radmmm_mpdh3_unframe(const float* dF, const float* add, const float* X, float* dZ, void* dZh, void* dZl, int ldh, int S,
                          int H, int C, int Ho, int stride, float slope, int rows_pad, float scale, int32_t* sat_flag,
                          radmmm_stream_t stream);
int radmmm_mpdh3_conv_post_dgrad(const float* dOut, const float* W, const float* add, const float* X, float* dZ, void* dZh,
                                  void* dZl, int ldh, int B2, int p, int H, int C, float slope, int rows_pad, float scale,
                                  int32_t* sat_flag, radmmm_stream_t stream);
int radmmm_mpdh3_plan(int S, int Hin, int Cin, int Hout, int Cout, int stride);

/* ------------------------------------------------------------------------------------
 * Grouped strided 1-d convolution on the fp32 matrix cores, forward and backward (additive entry points of ABI 4): the
 * kernel family of the HiFi-GAN multi-scale discriminator's five grouped 41-tap layers (hifigan_models.py: DiscriminatorS).
 * Geometry: S sequences, G groups, C_in = G*Cin_g, C_out = G*Cout_g, k taps (odd, <= 41), stride st in {1, 2, 4}, zero pad
 * k/2, Hout = (Hin-1)/st + 1; Cin_g and Cout_g multiples of 4 in [4, 64].  Anything else returns -1 before any HIP call.
 *   a PADDED map is [S][pad + H + pad][C] floats, the 2*pad outer rows of every sequence zero; X is padded by k/2, so
 *   window h' of group g is rows st*h' .. st*h' + k - 1, columns g*Cin_g .. (g+1)*Cin_g of X;  a DENSE matrix is [S*H][C];
 *   W is packed [G][Cout_g][k*Cin_g], kk = tap*Cin_g + ci  (torch's [C_out, Cin_g, k] permuted to [C_out, k, Cin_g]).
 * lrelu(v) = v > 0 ? v : slope*v; its derivative is taken from the saved OUTPUT y: y > 0 ? 1 : slope.
 *   msd_gconv_fwd    Y[s][pad_out + h'][g*Cout_g + co] = lrelu(bias[g*Cout_g + co] + sum_kk X[s][st*h' + tap][g*Cin_g + ci] *
 *                    W[g][co][kk]); Y is padded by pad_out (0 .. 20: the NEXT conv's k/2) and its pad rows are written as
 *                    zeros.  One launch covers all groups; no frame matrix is written.  slope 1 leaves the sum as it is.
 *   msd_gconv_dgrad  dX[(s*Hin + h)*C_in + g*Cin_g + ci] = (sum over the windows h' (ascending) and taps with st*h' + tap =
 *                    h + k/2 of sum_co dY[(s*Hout + h')*C_out + g*Cout_g + co] * W[g][co][tap*Cin_g + ci]
 *                    + add[s][h + k/2][..]) * lrelu'(X[s][h + k/2][..]).  dY, dX dense; add (X's padded layout, its pad
 *                    rows never read) may be NULL; X is the saved padded input map.
 *   msd_gconv_wgrad  P[split][g][co][tap*Cin_g + ci] = sum over the split's (s, h'), ascending, of
 *                    dZ[(s*Hout + h')*C_out + g*Cout_g + co] * X[s][st*h' + tap][g*Cin_g + ci].  The rows are cut into units
 *                    of 32 windows of one sequence; split i of n = msd_gconv_wgrad_splits(S, Hout, G, k) takes units
 *                    [i*U/n, (i+1)*U/n).  radmmm_colsum_final(P, dW, n, G*Cout_g*k*Cin_g) adds the splits.
 * Every contraction is a fixed chain of v_mfma_f32_16x16x4_f32; no atomics: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------ */
int radmmm_msd_gconv_fwd(const float* X, const float* W, const float* bias, float* Y, int S, int Hin, int Hout, int G, int Cin_g,
                         int Cout_g, int k, int stride, int pad_out, float slope, radmmm_stream_t stream);
int radmmm_msd_gconv_dgrad(const float* dY, const float* W, const float* add, const float* X, float* dX, int S, int Hin, int Hout,
                           int G, int Cin_g, int Cout_g, int k, int stride, float slope, radmmm_stream_t stream);
int64_t radmmm_msd_gconv_wgrad_splits(int S, int Hout, int G, int k);
int radmmm_msd_gconv_wgrad(const float* dZ, const float* X, float* P, int S, int Hin, int Hout, int G, int Cin_g, int Cout_g,
                           int k, int stride, radmmm_stream_t stream);

/* What surrounds the grouped convolutions in the multi-scale discriminator (hifigan_models.py: DiscriminatorS,
 * MultiScaleDiscriminator).  One member sees S = 2B sequences, s = sig*B + b, sig 0 real, 1 generated; its dense 5-tap and
 * conv_post layers are the multi-period entry points with p = 1 on maps padded by 2.
 *   msd_avgpool     AvgPool1d(4, 2, padding 2), count_include_pad: out[(sig*B + b)*To + j] = (x[2j-2] + x[2j-1] + x[2j] +
 *                   x[2j+1]) / 4 with x = 0 outside [0, T), To = T/2 + 1; both signals in one launch.
 *   msd_avgpool_bwd its adjoint in gather form: gx[n*ldx + t] = (g[n*To + t/2] + g[n*To + t/2 + 1]) / 4, the second term
 *                   only when t/2 + 1 < To; N rows.
 *   msd_frame15     the first conv's frame matrix: F[(s*T + t)*16 + j] = x_s[t - 7 + j] for j < 15 inside [0, T), else 0
 *                   (15 taps, zero pad 7, stride 1; column 15 pads the row to 16 floats).  A copy.
 *   msd_unframe15   its adjoint: g[n*ldg + u] = sum over j = 14 .. 0 with 0 <= u + 7 - j < T of dF[(n*T + u + 7 - j)*16 + j].
 *   msd_repad       X[s][r][c] = lrelu(Z[(s*H + r - pad)*ldz + c]) for pad <= r < pad + H, else 0  (mpd_repad with a pad
 *                   parameter, 0 .. 20).
 *   msd_fm_terms    mpd_fm_terms with p = 1 on a map [2B][pad + H + pad][C] (pad >= 0) or the dense output [2B][H] (pad < 0,
 *                   C == 1); partial count: mpd_fm_terms_parts(B, 1, H, C).
 *   msd_finish      mpd_finish with EIGHT maps (the seven convs and conv_post): off host [9], C and H host [8], cnt [9][B] (row
 *                   8 the output's positions), norm [9].
 *   msd_fm_grad     mpd_fm_grad with p = 1 and a pad parameter.
 *   msd_out_grad    mpd_out_grad with p = 1 in the eight-map form: f uses norm[7] and cnt[7], the adversarial terms norm[8]
 *                   and cnt[8]. */
int radmmm_msd_avgpool(const float* y, const float* y_hat, int ldy, float* out, int B, int T, radmmm_stream_t stream);
int radmmm_msd_avgpool_bwd(const float* g, float* gx, int ldx, int N, int T, radmmm_stream_t stream);
int radmmm_msd_frame15(const float* y, const float* y_hat, int ldy, float* F, int B, int T, radmmm_stream_t stream);
int radmmm_msd_unframe15(const float* dF, float* g, int ldg, int N, int T, radmmm_stream_t stream);
int radmmm_msd_repad(const float* Z, int ldz, float* X, int S, int H, int C, int pad, float slope, radmmm_stream_t stream);
int radmmm_msd_fm_terms(const float* X, const int32_t* cnt, float* part, int B, int H, int C, int pad, radmmm_stream_t stream);
int radmmm_msd_finish(const float* part, const int32_t* off, const int32_t* C, const int32_t* H, const float* out,
                      const int32_t* cnt, float* res, double* norm, int B, radmmm_stream_t stream);
int radmmm_msd_fm_grad(const float* X, const int32_t* cnt, const double* norm, const float* up, float* G, int B, int H, int C,
                       int pad, radmmm_stream_t stream);
int radmmm_msd_out_grad(const float* out, const int32_t* cnt, const double* norm, const float* up, float* dOut, int B, int H,
                        radmmm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADMMM_HIP_H */
