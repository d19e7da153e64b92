/*
 * s2svc_hip.h -- C ABI of libs2svc_hip.so: the MI355X (gfx950) kernels behind the seq2seq-vc
 * hot path (VTN / AAS-VC / Transformer-TTS forward+backward, AAS alignment search, losses,
 * optimiser, STFT->log-mel).
 *
 * The reference (unilight/seq2seq-vc) has no FFI layer: its hot path is stock torch ops called
 * from seq2seq_vc/modules/ and seq2seq_vc/losses/.  Each entry point below therefore names the
 * reference call site(s) it replaces (paths relative to the reference root, tag 2024_08_07).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked "host"; `stream` is a hipStream_t passed as void*;
 *   - every function returns 0 on success, <0 on error (s2svc_last_error() gives the message);
 *   - no function synchronises the device or allocates memory: callers own all buffers;
 *   - dtype codes: 0 = float32, 1 = bfloat16 (raw uint16 storage).  Activations are channel-last,
 *     contiguous (B, T, D).  Reductions / softmax / LN / BN statistics are fp32, MAS is fp64;
 *   - masks never exist as tensors: kernels take int32 per-utterance length vectors;
 *   - dropout: a mask is a pure function of (seed, element index) (SplitMix64 output function over seed + index/4, 16 bits per element); kernels read
 *     seed = *seed_base + seed_off, seed_base in device memory (may be NULL), so a captured hipGraph
 *     draws fresh masks on every replay and backward kernels regenerate masks instead of loading them.
 *   - absent rows (`int Tn, const int32_t* vlens`, ABI version 2): a captured training step allocates a (B, Tn, C) activation at a
 *     PADDED length Tn, the reference computes on the batch cropped to its longest utterance (models/vtn.py:208-214,
 *     models/aas_vc.py:523-524).  Entry points that mix along time or reduce over the batch take the B int32 lengths `vlens` in
 *     device memory (graph DATA): row r = b * Tn + t with t >= vlens[b] is ABSENT -- excluded from every sum and count, read
 *     as a convolution's zero padding, written as zero (outputs and data gradients).  vlens = NULL: every row is present.
 */
#ifndef S2SVC_HIP_H
#define S2SVC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* s2svc_last_error(void);
int s2svc_abi_version(void);
/* Measurement aid: launches `workgroups` x `threads` of a kernel that stores one word per workgroup into `sink_1024_words`
   (4 KB of device memory).  What a DEPENDENT launch costs on this stack whatever it does (bench.py "launch_floor_us"). */
int s2svc_launch_floor(int workgroups, int threads, void* sink_1024_words, void* stream);

/* Hand-off points inside a captured graph (the data-parallel backward pass: apex DDP's per-bucket hooks, bin/vc_train.py:423-431, have
   no counterpart in a graph): _record on a CAPTURING stream adds an event-record node (hipEventRecordExternal; returns 1), on an
   ordinary stream it is hipEventRecord (returns 0); _stream_wait_event issued after the graph's launch makes `stream` wait for that
   point of that launch.  `ev` is an opaque handle from _event_create (host memory). */
int s2svc_event_create(void** out /* host */);
int s2svc_event_destroy(void* ev);
int s2svc_event_record(void* ev, void* stream);
int s2svc_stream_wait_event(void* stream, void* ev);

/* ========================================================================================== */
/* Generic tiled MFMA GEMM with implicit-convolution operand addressing.                      */
/*   C[z][m,n] = act(alpha * sum_k A_z(m,k) * B_z(n,k) + bias[n]) + res_z[m,n]                 */
/* replaces: torch.nn.Linear / Conv1d / Conv2d / matmul call sites, e.g.                      */
/*   modules/transformer/attention.py:54-56,63,88,110 (QKV/out Linear, QK^T, PV)              */
/*   modules/transformer/positionwise_feed_forward.py:30-32                                   */
/*   modules/pre_postnets.py:63-66,108-185 (Prenet Linear, Postnet Conv1d)                    */
/*   modules/transformer/subsampling.py:58-70 (Conv2d 3x3 stride 2, Linear)                   */
/*   modules/alignments.py:21-26 (AlignmentModule Conv1d), length_regulator.py:153 (matmul)   */
/*   bin/preprocess.py:63-83 (STFT as windowed-DFT GEMM with overlapping rows, mel basis)     */
/* and their autograd backward (dgrad / wgrad are the same kernel with other operand layouts) */
/* ========================================================================================== */
enum { S2SVC_LAYOUT_KC = 0,   /* element (r,k) at r*ld + k  (reduction index contiguous)   */
       S2SVC_LAYOUT_RC = 1 }; /* element (r,k) at k*ld + r  (row index contiguous)          */
enum { S2SVC_OP_DENSE = 0,
       S2SVC_OP_CONV1D = 1,   /* rows/reduction index m=(b,t); taps j: x[(m+j-pad)*ld + c], valid iff 0<=t+j-pad<T */
       S2SVC_OP_CONV2D_S2 = 2,/* NHWC input (B,T1,F1,C), 3x3 stride 2 no padding, m=(b,t2,f2)  */
       /* A only, bf16 only: DATA gradient of that convolution for ONE parity class (pt, pf) of input pixels
          (t1, f1) = (2i+pt, 2j+pf): rows m = (b, i, j) over the class grid T1 x F1 (= ceil((T_in-pt)/2) x ceil((F_in-pf)/2)),
          reduction index k = tap*C + o over the (2-pt)*(2-pf) taps of the class, tap = ta*(2-pf) + fb reads the output-
          gradient pixel (i-ta, j-fb) of the (B,T2,F2,C) tensor (zero outside); pad = 2*pt + pf.  The weight operand is
          the class matrix s2svc_tconv2d_weights() lays out; use it with the c_map of s2svc_gemm_desc. */
       S2SVC_OP_TCONV2D_S2 = 3 };

typedef struct {
  const void* ptr;
  int64_t ld;
  int32_t layout;          /* S2SVC_LAYOUT_* */
  int32_t mode;            /* S2SVC_OP_*     */
  int32_t C;               /* conv: channels per tap (the implicit index is tap*C + c)        */
  int32_t T;               /* conv1d: frames per batch item                                   */
  int32_t pad;             /* conv1d: left padding (kernel-1)/2                               */
  int32_t T1, F1, T2, F2;  /* conv2d: input and output spatial dims                           */
  int64_t bs0, bs1;        /* two-level batch strides (elements)                              */
  int32_t zero_padded;     /* dense: the vectorised extent (k for KC, row for RC) is not a multiple of 16 bytes
                              but every row is padded with ZEROS up to one (ld covers it); lets the fast
                              kernels read whole vectors without masking                                */
  int32_t reserved_;
} s2svc_operand;

typedef struct {
  s2svc_operand A, B;
  void* C;
  int64_t ldc, cbs0, cbs1;
  int32_t c_dtype;         /* dtype of C / res                                                */
  const float* bias;       /* [N] fp32 or NULL                                                */
  const void* res;         /* residual added after activation, same dtype as C, or NULL       */
  int64_t ldr, rbs0, rbs1;
  int32_t M, N, K;
  int32_t nb0, nb1;        /* batch count = nb0*nb1 (>=1)                                     */
  int32_t act;             /* 0 none 1 relu 2 tanh 3 swish 4 sigmoid 5 gelu                   */
  float alpha;
  int32_t dtype;           /* dtype of A and B                                                */
  int32_t accumulate;      /* 1: C += result (C read in c_dtype)                              */
  int32_t splitk;          /* >1: partial sums go to ws[splitk][batch][M][N] fp32             */
  float* ws;
  /* optional fused row sums of A: a_rowsum[m] (+)= sum_k A(m,k)  (the bias gradient when A = dY^T in a   */
  /* wgrad GEMM); needs nb0*nb1 == 1; a_rowsum_ws: >= splitk*M floats when splitk > 1                     */
  float* a_rowsum;
  float* a_rowsum_ws;
  int32_t a_rowsum_accumulate;
  int32_t tile_hint;       /* 0 = auto, 64 or 128: output tile edge chosen by the caller's cost model */
  /* optional epilogue stage between the activation and the residual (needs nb0*nb1 == 1, ldc == N):               */
  /*   v *= dropout_scale(*seed_base + seed_off, m*N + n, drop_p)   -- the mask the standalone dropout kernels draw */
  /*   v  = emask[m*ldm + n] > 0 ? v : 0                            -- emask has the dtype of C                     */
  /* fuses `dropout(relu(x W1^T))` into the forward GEMM and `dY W2 * dropmask * relu'(h)` into the dgrad GEMM of   */
  /* positionwise_feed_forward.py:30-32, and relu' of subsampling.py:58-60 into the dgrad of the Linear after it.  */
  /*   emask_mode 1: v *= swish'(emask[m*ldm + n])  -- emask holds the PRE-activation of the forward pass (the data-gradient  */
  /*   GEMM through w_2 of a Swish feed-forward block then needs no element-wise pass either)                                  */
  const void* emask;
  int64_t ldm;
  float drop_p;
  int32_t emask_mode;
  const uint64_t* seed_base;
  uint64_t seed_off;
  /* c_map = 1 (bf16 LDS-DMA kernels only; no res / dropout / batch / split-K; emask: mode 0 only, indexed like C, i.e. by the
     MAPPED row -- relu' of the layer below fused into the transposed convolution): GEMM row m = (b, i, j) over the class grid
     cm_Tc x cm_Fc is stored at row (b*cm_T1 + 2i+cm_pt)*cm_F1 + 2j+cm_pf of C -- the four parity classes of a stride-2
     transposed convolution write one NHWC tensor (B, cm_T1, cm_F1, N) without a col2im pass */
  int32_t c_map;
  int32_t cm_T1, cm_F1, cm_Tc, cm_Fc, cm_pt, cm_pf;
  int32_t reserved3_;
  /* optional second output: alpha * A.B^T + bias BEFORE the activation (same dtype, ld and batch strides as C; no c_map) -- the
     pre-activation a Swish / GELU backward pass needs, written by the GEMM whose epilogue applies activation + dropout */
  void* c_pre;
} s2svc_gemm_desc;

int s2svc_gemm(const s2svc_gemm_desc* desc /* host */, void* stream);
/* Which kernel ran (tests): the name of the kernel instantiation that the most recent s2svc_gemm call of the calling thread launched,
   with the template arguments that tell the variants apart -- "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,5,lean>", "glds_k2<32,64,3>",
   "8ph_q<CONV1D,2,4>", "fast<f32,32,32,128,KC,KC>", "generic<bf16,64,64>", "skinny<bf16,1,lean>" -- followed by "+splitk_reduce" and /
   or "+stage_pass" when the call added those launches; "" when it launched nothing.  The name is set where the kernel is launched.  The
   string belongs to the library and holds until the thread's next call of this function. */
const char* s2svc_gemm_last_route(void);

/* Weight matrices of the four parity classes of the 3x3 stride-2 transposed convolution (S2SVC_OP_TCONV2D_S2), from the
   fp32 master weight w (O, C, 3, 3): out (bf16) = class (0,0) | (0,1) | (1,0) | (1,1), class (pt, pf) = [C][ntaps*O] with
   element [c][tap*O + o] = w[o, c, pt + 2*ta, pf + 2*fb], tap = ta*(2-pf) + fb; offsets 0, 4*C*O, 6*C*O, 8*C*O; 9*C*O total.
   Replaces the `col2im` half of autograd's conv2d input gradient (subsampling.py:58-63). */
int s2svc_tconv2d_weights(int O, int C, const float* w, void* out_bf16, void* stream);

/* Grouped launch of independent weight-gradient GEMMs  dW[N_out, N_in] (+)= dY^T . X  (bf16, both operands dense and
   row-contiguous -- what the backward of every Linear / 1x1 Conv1d issues; replaces the per-layer torch.nn.Linear weight
   gradients autograd computes one by one behind trainers/ar_vc.py:99 `loss.backward()`).  The host queues the
   descriptors of a few consecutive layers during backward and launches them as ONE grid: every workgroup runs the whole
   reduction of its output tile, so there is no split-K workspace and no reduction pass.
     _ok : 1 if `desc` can join a group (else launch it with s2svc_gemm);
     s2svc_gemm_grouped : `descs` is a HOST array; descriptors travel by value in the kernel arguments (10 per launch,
           n problems take ceil(n / 10) launches; hipGraph capture records them with the nodes), `tile` = 64 or 128 is the
           output tile edge, every descriptor must have splitk <= 1.
   Two descriptors of one call must not write the same C / a_rowsum (they run concurrently). */
int s2svc_gemm_grouped_ok(const s2svc_gemm_desc* desc /* host */);
int s2svc_gemm_grouped(const s2svc_gemm_desc* descs /* host */, int n, int tile, void* stream);
/* BATCHED problems of one operand-kind pair (A K-contiguous or row-contiguous, B row-contiguous; bf16, no split-K) as one
   grid: the batched products of an attention backward pass (ops/functional.py: _attn_common_bwd, _RelAttnPacked.backward;
   reference modules/transformer/attention.py:72-111, 262-305 differentiated).  0 = launched, 1 = not eligible as a group
   (nothing launched: run them with s2svc_gemm), < 0 = error. */
int s2svc_gemm_grouped_batched(const s2svc_gemm_desc* descs /* host */, int n, void* stream);
/* RAGGED weight gradients on the 8-wave kernel (csrc/gemm_8ph.hip, "W8"): C[M, N] fp32 (+)= A^T . B for dense row-contiguous bf16
   operands with M % 8 == N % 8 == 0 and ANY K (the Linear weight gradients dW = dY^T . X of the backward pass,
   /root/reference trainers/ar_vc.py:99-107: loss.backward() fills every parameter's .grad), as ONE grid of (problem, K chunk,
   256 x 128 tile) units, up to 40 problems per launch.  A reduction longer than 64 K tiles of 64 rows is cut into chunks -- a
   function of K only -- whose fp32 partial tiles go through `ws` and are added in chunk order by a second launch (deterministic).
     _ok        : 1 if the kernel takes `desc` (a function of the descriptor only).  Since round 4 that includes the exact-256
                  problems with >= 64 tiles of 128 x 128 (AAS-VC's decoder layers);
                  Round 5: B may also be the implicit im2col operand of a convolution weight gradient (S2SVC_LAYOUT_RC with
                  S2SVC_OP_CONV2D_S2 or S2SVC_OP_CONV1D, C % 128 == 0, whole images / utterances in K; Conv1d only for outputs of
                  >= 64 tiles) -- replaces autograd's conv weight gradients at subsampling.py:58-63 and alignments.py:28-60;
                  at most one convolution geometry per _grouped call;
     _ws_floats : fp32 elements of workspace the listed problems need (0 = none);
     _grouped   : launch; `ws` device memory (16-byte aligned) the caller keeps untouched until the launches have run. */
int s2svc_gemm_wgrad_ok(const s2svc_gemm_desc* desc /* host */);
int64_t s2svc_gemm_wgrad_ws_floats(const s2svc_gemm_desc* descs /* host */, int n);
int s2svc_gemm_wgrad_grouped(const s2svc_gemm_desc* descs /* host */, int n, float* ws, void* stream);
/* the same on a CAPPED grid: at most `wgs_cap` workgroups walk the units in order and leave the rest of the chip to the kernels of
   the stream the launch runs beside (forked gradient batches); same sums, same bits (wgs_cap <= 0: one workgroup per unit) */
int s2svc_gemm_wgrad_grouped_bg(const s2svc_gemm_desc* descs /* host */, int n, float* ws, void* stream, int wgs_cap);
/* A/B switch (tests, benchmarks): on = 0 / 1 (< 0: unchanged), kt_chunk = K tiles of 64 rows per chunk (<= 0: unchanged; default 64);
   returns the previous on | kt_chunk << 8. */
int s2svc_gemm_set_w8(int on, int kt_chunk);

/* Kernel-family switch for tests / A-B timing of s2svc_gemm's bf16 path: the 256-row, 8-wave, phase-interleaved kernel
   (csrc/gemm_8ph.hip: K-contiguous dense or Conv2d-3x3-s2 A operand, dense B, K % 64 == 0, >= 128 tiles) is tried first.
   mode & 15: 0 = never, 1 = default policy, 2 = policy without the half-phase skew of the two wave halves;
   (mode >> 4) & 15: 0 = tile geometry by policy, 1 = 256 x 256, 2 = 512 x 128, 3 = 256 x 128 forced (eligible problems only);
   (mode >> 8) & 15: 0 = unchanged, 1 + v sets the 256 x 96 p one-round geometry (gemm_8ph_kernel_n96): v = 0 never,
   1 by policy (default), 2 wherever N % 96 p == 0 (widest p), 4 / 5 = the same with p = 2 / 3 only.
   Returns the previous mode (mode < 0: query only).  Results do not depend on the mode beyond fp32 summation order. */
int s2svc_gemm_set_8ph(int mode);

/* ========================================================================================== */
/* LayerNorm fused with residual-add + dropout; BatchNorm1d; deterministic column reductions  */
/* replaces: modules/transformer/layer_norm.py:12-42 and the `residual + dropout(...)` lines   */
/* of encoder_layer.py:96-113, decoder_layer.py:104-127, conformer/encoder_layer.py:118-170;  */
/* torch.nn.BatchNorm1d at pre_postnets.py:124,152 and conformer/convolution.py:52,74.        */
/* ========================================================================================== */
/* s = res ? res + hscale*dropout(x) : x (written to s_out) ; y = LN(s)*gamma+beta ; mean/rstd [rows] fp32 */
int s2svc_layernorm_fwd(int dtype, int rows, int D, const void* x, const void* res, float drop_p, float hscale,
                        const uint64_t* seed_base, uint64_t seed_off, const float* gamma, const float* beta, float eps,
                        void* y, void* s_out, float* mean, float* rstd, void* stream);
/* ds = dLN(dy) + ds_extra ; dh = ds*mask*hscale (NULL to skip) */
int s2svc_layernorm_bwd(int dtype, int rows, int D, const void* dy, const void* s, const float* mean, const float* rstd,
                        const float* gamma, const void* ds_extra, float drop_p, float hscale, const uint64_t* seed_base,
                        uint64_t seed_off, void* ds, void* dh, void* stream);
/* chunked column reductions over (rows, D); modes 0..6 see csrc/norm.hip (5: sum dy, sum dy*v[r] with v in `mean`; 6: sum x, sum x^2); ws >= ws_chunks*2*D floats */
int s2svc_colreduce(int dtype, int rows, int D, int mode, const void* dy, const void* x, const float* mean,
                    const float* rstd, float scale, float* out_sum, float* out_dot, int accumulate, float* ws,
                    int ws_chunks, int Tn, const int32_t* vlens /* absent rows; scale < 0: 1 / number of present rows */, void* stream);
/* Several column reductions in two launches (stage 1, stage 2): the parameter gradients of the LayerNorm / BatchNorm /
   bias vectors of a few consecutive layers, queued by the host during backward.  Same semantics per item as
   s2svc_colreduce (ws >= ws_chunks*2*D floats each).  Two items of one call must not write the same out_sum / out_dot. */
typedef struct {
  const void* dy;
  const void* x;
  const float* mean;
  const float* rstd;
  float* out_sum;
  float* out_dot;
  float* ws;
  int32_t dtype, rows, D, mode, accumulate, ws_chunks;
  float scale;
  int32_t reserved_;
} s2svc_colreduce_item;
int s2svc_colreduce_grouped(const s2svc_colreduce_item* items /* host */, int n, void* stream);
/* LayerNorm backward (layer_norm.py:12-42 under autograd) together with the FIRST reduction stage of its parameter gradients
   (round 4): the launch also writes `chunks` partial row pairs ws[chunk][2][D] (sum of dy | sum of dy * xhat over the chunk's
   rows), which enter s2svc_colreduce_grouped as an item of mode 7 (partials ready: ws, ws_chunks = chunks, D, out_sum = d beta,
   out_dot = d gamma).  _pg_chunks: 0 = not eligible (use s2svc_layernorm_bwd and a mode-1 reduction), else the chunk count. */
int s2svc_layernorm_bwd_pg_chunks(int dtype, int rows, int D, const void* dy, const void* s, const float* gamma, const void* ds_extra,
                                  const void* ds, const void* dh);
int s2svc_layernorm_bwd_pg(int dtype, int rows, int D, const void* dy, const void* s, const float* mean, const float* rstd,
                           const float* gamma, const void* ds_extra, float drop_p, float hscale, const uint64_t* seed_base,
                           uint64_t seed_off, void* ds, void* dh, float* ws, void* stream);
int s2svc_bn_finalize(int C, int n, float eps, float momentum, const float* mean, const float* var, float* rstd,
                      float* run_mean, float* run_var, int64_t* num_batches, int var_is_ex2 /* var = E[x^2], colreduce mode 6 */,
                      int Tn, const int32_t* vlens /* absent rows: n = B * Tn -> the number of present rows */, void* stream);
int s2svc_rstd_from_var(int C, float eps, const float* var, float* rstd, void* stream);
/* The training-mode statistics of torch.nn.BatchNorm1d (pre_postnets.py:124,152, conformer/convolution.py:52,74) with the second
   reduction stage folded into the finalisation: 2 launches instead of 3 (ws >= ws_chunks*2*C floats).
   s2svc_bn_stats == s2svc_colreduce(mode 6, scale 1/rows) + s2svc_bn_finalize(var_is_ex2 = 1). */
int s2svc_bn_stats(int dtype, int rows, int C, const void* x, float eps, float momentum, float* mean, float* rstd,
                   float* run_mean, float* run_var, int64_t* num_batches, float* ws, int ws_chunks, int Tn, const int32_t* vlens,
                   void* stream);
int s2svc_bn_apply(int dtype, int64_t rows, int C, const void* x, const float* mean, const float* rstd,
                   const float* gamma, const float* beta, int act, float drop_p, const uint64_t* seed_base,
                   uint64_t seed_off, void* y, void* pre_act, int Tn, const int32_t* vlens, void* stream);
int s2svc_bn_bwd(int dtype, int64_t rows, int C, const void* dy, const void* x, const float* mean, const float* rstd,
                 const float* gamma, const float* sum_dy, const float* sum_dy_xhat, int use_batch_stats, void* dx,
                 int Tn, const int32_t* vlens, void* stream);

/* ========================================================================================== */
/* Attention probabilities: scale + relative shift + length/causal mask + softmax + dropout   */
/* replaces: modules/transformer/attention.py:63-93 (forward_attention), :237-260 / :142-160  */
/* (rel_shift new / legacy), :278-303 ((ac+bd)/sqrt(d_k)).  rel_mode 0 none, 1 new, 2 legacy. */
/* ========================================================================================== */
/* score / probability rows are `ld` >= T2 elements apart (rows padded to a vector multiple); pad columns are written as 0; */
/* rows of the relative-position term bd / dbd (length Lp) are `ldb` >= Lp elements apart (dbd pad columns are written as 0); */
/* the forward and the backward both refuse ld < T2 and ldb < Lp before any launch                                          */
int s2svc_attn_softmax_fwd(int dtype, int B, int H, int T1, int T2, int ld, const float* scores, const float* bd, int Lp,
                           int ldb, int rel_mode, float scale, const int32_t* klen, int causal, float drop_p,
                           const uint64_t* seed_base, uint64_t seed_off, void* attn, void* pdrop, void* stream);
int s2svc_attn_softmax_bwd(int dtype, int B, int H, int T1, int T2, int ld, const void* attn, const float* dp, const void* dattn,
                           float scale, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* dscores,
                           void* dbd, int Lp, int ldb, int rel_mode, void* stream);

/* ========================================================================================== */
/* Elementwise: activations+dropout, positional encodings, head biases, GLU, casts, gathers   */
/* replaces: F.dropout / nn.Dropout sites (pre_postnets.py:63-66 always-on prenet dropout),   */
/* layers/positional_encoding.py:57-70,94-106,226-235,293-309, attention.py:283-286,          */
/* conformer/convolution.py:68 (GLU), conformer/swish.py.                                     */
/* ========================================================================================== */
int s2svc_act_dropout_fwd(int dtype, int64_t n, const void* x, int act, float p, const uint64_t* seed_base,
                          uint64_t seed_off, void* y, void* stream);
int s2svc_act_dropout_bwd(int dtype, int64_t n, const void* dz, const void* saved, int act, float p,
                          const uint64_t* seed_base, uint64_t seed_off, void* dx, void* stream);
int s2svc_posenc_fwd(int dtype, int64_t B, int T, int D, const void* x, float xscale, const float* alpha, const float* pe,
                     float p, const uint64_t* seed_base, uint64_t seed_off, void* y, void* stream);
int s2svc_posenc_bwd(int dtype, int64_t B, int T, int D, const void* dy, float xscale, const float* pe, float p,
                     const uint64_t* seed_base, uint64_t seed_off, void* dx, float* dalpha, float* partials, void* stream);
int s2svc_axpby(int dtype, int64_t n, float a, const void* x, float b, const void* y, void* out, void* stream);
/* ---- scalar / index glue of a training step (csrc/glue.hip): what sits between the fused kernels, one small launch each ---- */
#define S2SVC_SCALAR_TERMS_MAX 8
typedef struct {
  const float* x[S2SVC_SCALAR_TERMS_MAX]; /* term i: n[i] fp32 values (a scalar: n = 1) */
  int32_t n[S2SVC_SCALAR_TERMS_MAX];
  float w[S2SVC_SCALAR_TERMS_MAX];
  int32_t k;                              /* number of terms */
  int32_t reserved_;
} s2svc_scalar_terms;
/* *out = sum_i w[i] * sum_j x[i][j]: the training loss from its parts (trainers/aas_vc.py:100-139), means over the batch
   (forward_sum_loss.py:70-76, alignments.py:303-309); one wavefront, fixed order. */
int s2svc_weighted_sum(const s2svc_scalar_terms* terms /* host */, float* out, void* stream);
/* its backward: x[i][j] (written!) = w[i] * *g */
int s2svc_weighted_sum_bwd(const s2svc_scalar_terms* grads /* host; x[] are the OUTPUT buffers */, const float* g, void* stream);
/* acc[i] = beta * acc[i] + w[i] * sum_j x[i][j]: the running sums of the logged losses (trainers/base.py:198-213) */
int s2svc_scalars_axpy(const s2svc_scalar_terms* terms /* host */, float beta, float* acc, void* stream);
int s2svc_fill_zero(void* p, int64_t nbytes, void* stream);
/* *seed += inc (the device-resident dropout seed base, one bump per step) */
int s2svc_seed_advance(uint64_t* seed, uint64_t inc, void* stream);
/* out (rows, ldo) = [in (rows, N) | zeros] */
int s2svc_pad_cols(int dtype, int64_t rows, int N, int ldo, const void* in, void* out, void* stream);
/* teacher-forcing input of the AR decoder (models/vtn.py:236-243): out[b, t, :] = t == 0 ? 0 : ys[b, t * r - 1, :], ys fp32 with
   batch stride ys_batch_stride elements, out (B, Tin, D) in out_dtype */
int s2svc_decoder_input(int out_dtype, int B, int Tin, int r, int D, int64_t ys_batch_stride, const float* ys, void* out, void* stream);
/* token batch with <eos> behind every sequence (models/transformer_tts.py:139-142): out (B, T + 1) = [xs[b, :lens[b]] | eos | pad ...] */
int s2svc_append_eos(int B, int T, int64_t ldx, const int64_t* xs, const int32_t* lens, int64_t eos, int64_t pad, int64_t* out, void* stream);
/* out (rows, D) dense = src (rows, D) with row stride lds */
int s2svc_copy_rows(int dtype, int64_t rows, int D, int64_t lds, const void* src, void* out, void* stream);
/* stop-token targets (models/vtn.py:253-260): out (B, T) = labels (row stride ld_labels) with a 1 at frame lens[b] - 1 */
int s2svc_stop_labels(int B, int T, int64_t ld_labels, const float* labels, const int32_t* lens, float* out, void* stream);
/* out = x0 + x1 (+ x2 (+ x3)), k = 2..4 inputs summed in that order (fp32 arithmetic): the gradients arriving at a tensor with several
   consumers, in one launch (what autograd's accumulation does with k - 1 element-wise adds). */
int s2svc_add_n(int dtype, int64_t n, int k, const void* x0, const void* x1, const void* x2, const void* x3, void* out, void* stream);
int s2svc_add_head_bias(int dtype, int64_t rows, int D, const void* q, const float* u, const float* v, void* qu, void* qv,
                        void* stream);
/* the same with q a column block of a packed Q|K|V projection (row stride ldq elements); qu, qv dense (rows, D) */
int s2svc_add_head_bias_ld(int dtype, int64_t rows, int D, const void* q, int64_t ldq, const float* u, const float* v, void* qu,
                           void* qv, void* stream);
/* out[r, :D] = a[r, :D] + b[r, :D] over row-strided views (e.g. dQ = dQu + dQv written into the packed gradient) */
int s2svc_add_rows(int dtype, int64_t rows, int D, const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo,
                   void* stream);
int s2svc_glu_fwd(int dtype, int64_t rows, int C, const void* x, void* y, void* stream);
int s2svc_glu_bwd(int dtype, int64_t rows, int C, const void* x, const void* dy, void* dx, void* stream);
int s2svc_cast(int in_dtype, int out_dtype, int64_t n, const void* x, void* y, void* stream);
int s2svc_gather3(int in_dtype, int out_dtype, int n0, int n1, int n2, int64_t s0, int64_t s1, int64_t s2, int64_t off,
                  const void* in, void* out, void* stream);
/* Several gathers of fp32 sources in one launch: the permuted compute-dtype copies of the convolution weights
   ((O, I, k) -> (O, k, I) for the implicit-GEMM forward, (I, k reversed, O) for the data gradient, ...), refreshed once
   after the optimiser step instead of one launch per layer and pass inside the step.  `jobs` is a HOST array. */
typedef struct s2svc_gather3_job {
  const void* in;      /* fp32 */
  void* out;           /* contiguous n0 x n1 x n2, out_dtype */
  int64_t s0, s1, s2, off;
  int32_t n0, n1, n2;
  int32_t out_dtype;
} s2svc_gather3_job;
int s2svc_gather3_grouped(const s2svc_gather3_job* jobs /* host */, int n, void* stream);
/* Every derived copy of the weights in ONE launch (up to 48 jobs; one more launch per further 48), what the optimiser runs
   after each update: the gathers above (kind GATHER3, fields as in s2svc_gather3_job) and the class matrices of the stride-2
   transposed convolution (kind TCONV2D: in = fp32 weight (O, C, 3, 3), out = bf16, 9*C*O elements in the layout of
   s2svc_tconv2d_weights, n0 = O, n1 = C; strides, off and n2 unused).  The work of all jobs is cut into units (an LDS tile
   or a 4096-element slice) that are spread evenly over the grid; a job whose source and output both have a unit-stride
   direction is read and written in contiguous runs through LDS.  A copy plus at most one fp32 -> bf16 rounding: the results
   are those of s2svc_gather3 / s2svc_tconv2d_weights bit for bit.  `jobs` is a HOST array.
   _plan (host only, no device needed): the path (0 element-wise, 1 tile, 2 slab, 3 class-matrix tile) and the number of
   units of every job, as the launch would take them. */
enum { S2SVC_DERIVED_GATHER3 = 0, S2SVC_DERIVED_TCONV2D = 1 };
typedef struct s2svc_derived_job {
  const void* in;      /* fp32 */
  void* out;
  int64_t s0, s1, s2, off;
  int32_t n0, n1, n2;
  int32_t out_dtype;
  int32_t kind;        /* S2SVC_DERIVED_* */
  int32_t reserved_;
} s2svc_derived_job;
int s2svc_derived_refresh(const s2svc_derived_job* jobs /* host */, int n, void* stream);
int s2svc_derived_refresh_plan(const s2svc_derived_job* jobs /* host */, int n, int32_t* path /* host, n */, int32_t* units /* host, n */);
/* dst[o][b][a] (+)= src[o][a][b], fp32, o < n: a convolution weight gradient (C_out, taps, C_in) as the GEMM leaves it into the
   parameter's (C_out, C_in, taps) layout (replaces the transposes autograd does inside conv backward: subsampling.py:58-63,
   pre_postnets.py:108-165, alignments.py:28-60 call sites).  A * (B + 1) * 4 bytes must fit 64 KB. */
int s2svc_permute_inner(int n, int A, int B, const float* src, float* dst, int accumulate, void* stream);
int s2svc_rowscale(int dtype, int64_t rows, int D, const void* x, const float* s, void* out, void* stream);
/* Weight gradients of 'same'-padded stride-1 Conv1d layers without bias, several layers in ONE launch (csrc/conv1d_wgrad.hip; replaces
   the split-K GEMM + reduction + permutation of autograd's conv backward at the pre_postnets.py:108-165 call sites):
     dw[o][i][j] += sum_{b,t} dy[b,t,o] * x[b, t + j - (ks-1)/2, i],   taps outside [0, T) of the same utterance count as zero.
   dy (B*T, Cout) and x (B*T, Cin) are row-major bf16, 16-byte aligned; dw is fp32 in the parameter's (Cout, Cin, ks) layout and is ADDED
   to.  Supported: dtype 1 (bf16), ks = 5, Cin and Cout multiples of 16.  A unit is (item, 64 output channels, 64 input channels, all
   taps) and sums all B*T rows in ascending order in one accumulator set; workgroups walk the units in order, so the result is bit-identical
   for every max_workgroups (0 = one workgroup per unit).  Items whose dw ranges overlap go to successive launches, as do items beyond 16.
   chunk_steps > 0: the frames are summed in runs of chunk_steps 64-frame steps (utterance by utterance, ceil(T / 64) steps each), every
   run from zero, the runs added in ascending order: with T % 64 == 0 and chunk_steps = ceil(B*T / 64 / splitk) these are the partial
   sums and the reduction of an s2svc_gemm with that split-K, bit for bit -- as long as that GEMM runs 64-row K tiles on the 16x16x32 bf16
   MFMA (gemm_glds_kernel with row-contiguous operands) and splitk_reduce adds its partials in ascending order; this entry point
   promises the formula and the order stated here, not that equality.  0: one run.  Every argument is checked before the first launch. */
typedef struct s2svc_conv1d_wgrad_item {
  const void* dy;
  const void* x;
  float* dw;
  int32_t B, T, Cin, Cout, ks;
  int32_t dtype;
  int32_t chunk_steps;
  int32_t reserved_;
} s2svc_conv1d_wgrad_item;
int s2svc_conv1d_wgrad_supported(int Cout, int Cin, int ks, int dtype);
int s2svc_conv1d_wgrad_grouped(const s2svc_conv1d_wgrad_item* items /* host */, int n, int max_workgroups, void* stream);

/* ========================================================================================== */
/* Convolution helpers                                                                         */
/* replaces: autograd of Conv2d stride 2 (subsampling.py:58-63); F.interpolate (aas_vc.py:    */
/* 340-349); depthwise Conv1d (conformer/convolution.py:42-51,70; vits/flow.py:137-146).      */
/* ========================================================================================== */
/* first front-end layer: Conv2d(1->O, 3x3, s2) + ReLU on the (B,T,F) mel batch, output NHWC; fused dW + dbias */
int s2svc_conv_in1_fwd(int dtype, int B, int Tn, int Fn, int O, const void* x, const float* w, const float* bias, void* y,
                       void* stream);
/* y != NULL: dy is the gradient of the ReLU output and is masked by (y > 0) on the fly */
int s2svc_conv_in1_wgrad(int dtype, int B, int Tn, int Fn, int O, const void* x, const void* dy, const void* y, float* dw,
                         float* db, int accumulate, float* partial, int max_chunks, void* stream);
int s2svc_col2im_s2(int dtype, int B, int T1, int F1, int C, int T2, int F2, const void* dcols, void* dx, void* stream);
/* ext_in / ext_out (device, one int32 each, or NULL): the lengths the reference's cropped tensors have when Tin / Tout are padded
   lengths of a captured step -- they set the resampling ratio; output frames >= *ext_out are zero, input frames >= *ext_in unread. */
int s2svc_interp_nearest(int dtype, int B, int Tin, int Tout, int C, const void* x, void* y, const int32_t* ext_in,
                         const int32_t* ext_out, void* stream);
int s2svc_interp_nearest_bwd(int dtype, int B, int Tin, int Tout, int C, const void* dy, void* dx, const int32_t* ext_in,
                             const int32_t* ext_out, void* stream);
/* The same resampling with one pair of lengths PER ROW (lens_in / lens_out: B int32 each, device) -- inference on a padded batch of
   utterances of different lengths (AASVC.inference_batch): replaces the per-utterance F.interpolate of models/aas_vc.py:345-350 with
   each row's own ratio lens_in[b] / lens_out[b]; output frames >= lens_out[b] are zero, input frames >= lens_in[b] never read.  No backward. */
int s2svc_interp_nearest_rows(int dtype, int B, int Tin, int Tout, int C, const void* x, void* y, const int32_t* lens_in,
                              const int32_t* lens_out, void* stream);
int s2svc_dwconv(int dtype, int B, int Tn, int C, int ks, int dil, const void* x, const float* w, const float* bias,
                 void* y, int flip, void* stream);
/* y = dwconv(x) + add (add: a tensor of y's shape or NULL): the data gradient of a depthwise convolution whose input also feeds a
   residual connection (flow.py:148-190) takes the residual's gradient along instead of a separate add. */
int s2svc_dwconv_add(int dtype, int B, int Tn, int C, int ks, int dil, const void* x, const float* w, const float* bias,
                     const void* add, void* y, int flip, void* stream);
int s2svc_dwconv_wgrad(int dtype, int B, int Tn, int C, int ks, int dil, const void* x, const void* dy, float* dw,
                       int accumulate, float* ws, int ws_chunks, void* stream);

/* Core of the Conformer convolution module in training mode, bf16 (csrc/convmod.hip):
   GLU -> depthwise conv -> BatchNorm1d batch statistics -> Swish between the two pointwise convolutions.
   replaces: modules/conformer/convolution.py:68-75 (glu, depthwise_conv, norm, activation) and their autograd backward.
     y2 (B,Tn,2C) bf16 = output of pointwise_conv1;  w (C,1,ks) fp32, bias (C) or NULL;  z (B,Tn,C) bf16 = depthwise_conv(glu(y2));
     mean / rstd (C): batch statistics of z over all B*Tn frames (padded frames included, like the reference); run_mean / run_var /
     num_batches: torch.nn.BatchNorm1d's running buffers (may be NULL);  ws >= B * ceil(Tn / 64) * 2 * C floats.
   s2svc_convmod_supported: C % 64 == 0 and ks in {7, 15, 31}; everything else takes the separate kernels. */
int s2svc_convmod_supported(int C, int ks);
int s2svc_convmod_fwd(int B, int Tn, int C, int ks, const void* y2, const float* w, const float* bias, void* z, float eps,
                      float momentum, float* mean, float* rstd, float* run_mean, float* run_var, int64_t* num_batches, float* ws,
                      const int32_t* vlens, void* stream);
/* out = swish((z - mean) * rstd * gamma + beta), bf16, C % 64 == 0 */
int s2svc_bn_swish_apply(int64_t rows, int C, const void* z, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, void* out, int Tn, const int32_t* vlens, void* stream);
/* da (B,Tn,C) bf16 = gradient of the Swish output -> dy2 (B,Tn,2C) bf16 = gradient of y2;  sdy / sdyx (C) = gradients of the
   BatchNorm bias / weight (also ADDED to dbeta_acc / dgamma_acc when given);  ws_w receives the per-tile partial sums of the
   depthwise weight and bias gradients, [B * ceil(Tn / 64)][C][ks + 1] (s2svc_convmod_wgrad_final sums them);
   ws_stats >= ceil(B * Tn / 64) * 2 * C floats. */
int s2svc_convmod_bwd(int B, int Tn, int C, int ks, const void* da, const void* z, const void* y2, const float* w, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, void* dy2, float* sdy, float* sdyx,
                      float* dgamma_acc, float* dbeta_acc, float* ws_stats, float* ws_w, const int32_t* vlens, void* stream);
int s2svc_convmod_wgrad_final(int C, int ks, int chunks, const float* ws_w, float* dw, float* db, int accumulate, void* stream);

/* Core of the Conformer convolution module in INFERENCE mode, fp32 or bf16, one launch, per-row lengths (csrc/convmod_infer.hip):
   GLU -> depthwise conv -> BatchNorm1d with its running statistics -> Swish between the two pointwise convolutions.
   replaces: modules/conformer/convolution.py:68-75 (glu, depthwise_conv, norm, activation) in eval().
     y2 (B,Tn,2C) = output of pointwise_conv1 in `dtype`;  w (C,1,ks) fp32, bias (C) or NULL;  run_mean / run_var (C);  gamma / beta (C) or
     NULL (1 / 0);  out (B,Tn,C) in `dtype`;  vlens (B int32) or NULL (every row is full):
       out[b,t,c] = swish(((bias[c] + sum_j w[c,j] g[b,t+j-(ks-1)/2,c]) - run_mean[c]) / sqrt(run_var[c] + eps) * gamma[c] + beta[c]),  t < vlens[b]
       out[b,t,c] = 0,  t >= vlens[b];      g = glu(y2) at frames 0 <= t' < vlens[b], 0 elsewhere.
     Frames >= vlens[b] of y2 are never read (they may hold anything, NaN included); every element of out is written exactly once;
     fp32 accumulation in a fixed order, no atomics, no workspace.  y2 and out 16-byte aligned, B * ceil(Tn / 64) <= 65535.
   s2svc_convmod_infer_supported: C % 8 == 0 and odd ks <= 31; everything else takes the separate kernels. */
int s2svc_convmod_infer_supported(int C, int ks);
int s2svc_convmod_infer(int dtype, int B, int Tn, int C, int ks, const void* y2, const float* w, const float* bias, const float* run_mean,
                        const float* run_var, const float* gamma, const float* beta, float eps, void* out, const int32_t* vlens,
                        void* stream);

/* BatchNorm1d (training mode) + activation + dropout on channel-last bf16 rows, C % 8 == 0, 16-byte accesses (csrc/batchnorm.hip).
   replaces: modules/pre_postnets.py:108-165 (BatchNorm1d -> Tanh -> Dropout of the Postnet layers) and its autograd backward.
     s2svc_bn_stats_vec: mean / rstd over (rows, C) + torch's running statistics; ws >= ceil(rows / 64) * 2 * C floats.
     s2svc_bn_act_apply_vec: y = dropout(act((x - mean) * rstd * gamma + beta)); pre_act (or NULL) = the value before act.
     s2svc_bn_act_bwd_vec: dz = d y; saved = y (relu / tanh / sigmoid) or pre_act (swish / gelu), NULL for act none and no dropout;
       -> dx, sdy = d beta, sdyx = d gamma (also ADDED to dbeta_acc / dgamma_acc when given).  The activation / dropout derivative is
       recomputed in both passes (no intermediate tensor).  Dropout masks: element index = row * C + channel, as s2svc_bn_apply. */
int s2svc_bn_stats_vec(int rows, int C, const void* x, float eps, float momentum, float* mean, float* rstd, float* run_mean,
                       float* run_var, int64_t* num_batches, float* ws, int Tn, const int32_t* vlens, void* stream);
int s2svc_bn_act_apply_vec(int rows, int C, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           int act, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* y, void* pre_act, int Tn,
                           const int32_t* vlens, void* stream);
int s2svc_bn_act_bwd_vec(int rows, int C, const void* dz, const void* saved, const void* x, const float* mean, const float* rstd,
                         const float* gamma, int act, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* dx, float* sdy,
                         float* sdyx, float* dgamma_acc, float* dbeta_acc, float* ws, int Tn, const int32_t* vlens, void* stream);

/* ========================================================================================== */
/* AAS alignment: pairwise -L2 + masked log-softmax, monotonic alignment search, Gaussian     */
/* upsampling weights.                                                                         */
/* replaces: modules/alignments.py:51-59 (AlignmentModule tail), :63-93 + :281-310 (numba MAS, */
/* per-utterance host loop, bincount, binarisation loss), length_regulator.py:111-154.        */
/* ========================================================================================== */
int s2svc_pairwise_l2_logsoftmax(int dtype, int B, int Tf, int Tx, int A, const void* feats, const void* text,
                                 const int32_t* text_lens, float* logp, float* dist, void* stream);
int s2svc_pairwise_l2_bwd_g(int dtype, int B, int Tf, int Tx, const float* logp, const float* dist, const float* dlogp,
                            const int32_t* text_lens, void* G, float* rowsum, void* stream);
int64_t s2svc_mas_ws_bytes(int B, int Tf, int Tx);
/* path (B,Tf) int32 (-1 beyond feat_len), ds (B,Tx) fp32 durations, binmean (B) = mean_t log_p[t, path[t]] */
int s2svc_mas(int B, int Tf, int Tx, const float* log_p_attn, const int32_t* text_lens, const int32_t* feat_lens,
              int32_t* path, float* ds, float* binmean, void* ws, void* stream);
/* dlogp[b, t, path[b, t]] += -gout / (B * min(feat_lens[b], Tf)) for every path entry >= 0; B == 0 returns cleanly, Tf or Tx <= 0 is
   refused, as in s2svc_mas */
int s2svc_mas_binloss_bwd(int B, int Tf, int Tx, const int32_t* path, const int32_t* feat_lens, const float* gout,
                          float* dlogp, void* stream);
int s2svc_gauss_upsample_probs(int dtype, int B, int Tf, int Tx, const float* ds, const int32_t* text_lens,
                               const int32_t* feat_lens, float delta, void* P, void* stream);

/* Length regulator of FastSpeech-style models -- replaces modules/length_regulator.py:46-97 (per-utterance
   torch.repeat_interleave + pad_list): frame i of utterance b is repeated ds[b, i] times.
     _index: start (B,Tx) = exclusive prefix sums of ds, idx (B,Tout) = source frame of every output frame (-1 = padding),
             total (B) = sum of ds (may be NULL);   _fwd: y (B,Tout,D) = x[b, idx] or pad_value;
     _bwd:   dx (B,Tx,D) = sum of dy over each frame's run (fixed order, no atomics).
     Tout = 0 is a valid empty output: _index writes start / total only, _fwd returns without a launch, _bwd writes dx = 0
     (idx, y and dy of an empty output may be NULL). */
int s2svc_length_regulate_index(int B, int Tx, int Tout, const int32_t* ds, int32_t* start, int32_t* idx, int32_t* total,
                                void* stream);
int s2svc_length_regulate_fwd(int dtype, int B, int Tx, int Tout, int D, const void* x, const int32_t* idx, float pad_value,
                              void* y, void* stream);
/* Predicted durations -> the length regulator's input, per row of a padded batch, one wave per row (csrc/lenreg.hip).
   replaces: models/aas_vc.py:393 (clamp at MAX_DP_OUTPUT) + modules/length_regulator.py:127-135 (ds[ds.sum(dim=1).eq(0)] = 1 on the
   single-utterance tensor) + the two host reads of the duration sum that sized the output.
     d (B,Tx) fp32 (dtype_i64 = 0) or int64 (1), integers in value;  text_lens (B int32);  dmax: the clamp (dmax * Tx < 2^24);
     d_outs (B,Tx) in d's type = min(d, dmax), 0 at entries >= text_lens[b] (those entries of d are never read);
     ds (B,Tx) fp32 = d_outs, except that a row whose valid entries sum to 0 holds 1 in every VALID entry;  total (B int32) = row sums of ds. */
int s2svc_durations_finalize(int dtype_i64, int B, int Tx, const void* d, const int32_t* text_lens, float dmax, void* d_outs, float* ds,
                             int32_t* total, void* stream);
int s2svc_length_regulate_bwd(int dtype, int B, int Tx, int Tout, int D, const void* dy, const int32_t* start, const int32_t* ds,
                              void* dx, void* stream);
/* Durations from attention maps -- replaces utils/duration_calculator.py:13-65: att (NH, Tf, Tx) fp32 (NH = layers * heads,
   or 1); picks the head with the largest mean row maximum, durations[j] (int64) = number of frames whose arg-max is j;
   focus_rate / head (device scalars, may be NULL) = that head's score / index. */
int s2svc_attn_durations(int NH, int Tf, int Tx, const float* att, int64_t* durations, float* focus_rate, int32_t* head,
                         void* stream);

/* ========================================================================================== */
/* Losses                                                                                      */
/* replaces: losses/seq2seq_loss.py:30-59, losses/l1_loss.py:22-49, guided_attention_loss.py: */
/* 142-165, forward_sum_loss.py:26-116 (F.ctc_loss loop + scipy beta-binomial prior).          */
/* ========================================================================================== */
/* Empty problems are refused (rc -1, nothing launched or written) by each forward and its backward alike: B, Tm or D <= 0 for the
   sequence loss; B, H, To or Ti <= 0 or sigma <= 0 for the guided attention loss.  The guided attention kernels take ilens[b] > Ti /
   olens[b] > To as Ti / To, in the weights as in the count. */
int s2svc_seq_loss_fwd(int dtype, int B, int Tm, int D, const void* after, const void* before, const void* logits,
                       const float* ys, const float* labels, const int32_t* olens, float pos_weight, float* partial,
                       float* out, void* stream);
int s2svc_seq_loss_bwd(int dtype, int B, int Tm, int D, const void* after, const void* before, const void* logits,
                       const float* ys, const float* labels, const int32_t* olens, float pos_weight, const float* stats,
                       const float* g_l1, const float* g_bce, void* d_after, void* d_before, void* d_logits, void* stream);
int s2svc_guided_attn_loss_fwd(int dtype, int B, int H, int To, int Ti, const void* att, const int32_t* ilens,
                               const int32_t* olens, float sigma, float alpha, float* partial, float* out, void* stream);
int s2svc_guided_attn_loss_bwd(int dtype, int B, int H, int To, int Ti, const int32_t* ilens, const int32_t* olens,
                               float sigma, float alpha, const float* stats, const float* gout, void* datt, void* stream);
/* masked log-domain MSE of the deterministic duration predictor (losses/duration_predictor_loss.py:38-57);   */
/* stats[0] = number of valid tokens (kept for the backward)                                                 */
int s2svc_duration_loss_fwd(int B, int T, const float* d_outs, const float* ds, const int32_t* lens, float offset, int mean,
                            float* stats, float* out, void* stream);
int s2svc_duration_loss_bwd(int B, int T, const float* d_outs, const float* ds, const int32_t* lens, float offset, int mean,
                            const float* stats, const float* g, float* dd, void* stream);
int64_t s2svc_forward_sum_ws_bytes(int B, int Tf, int Tx);
int s2svc_forward_sum(int B, int Tf, int Tx, const float* log_p_attn, const float* prior, const int32_t* text_lens,
                      const int32_t* feat_lens, float log_blank, void* ws, float* loss_b, float* grad, void* stream);
int s2svc_betabinom_prior(int B, int Tf, int Tx, const int32_t* text_lens, const int32_t* feat_lens, float* prior,
                          void* stream);

/* ========================================================================================== */
/* Fused attention for short sequences (bf16, T1, T2 <= 64, d_k in {32,64,96,128}): one launch */
/* forward (scores, mask, softmax, dropout, P.V; writes the attention map) and one backward.   */
/* replaces: modules/transformer/attention.py:63-111 for VTN's shapes (T = 63/64, d_k = 96).   */
/* q/k/v/out/grads: element [b*bs + t*ld + h*dk + d] (bf16; slices of packed projections are   */
/* fine); attn / dattn: (B, H, T1, ld) bf16, T2 <= ld (forward: ld <= 64), pad columns [T2, ld) */
/* written as 0.                                                                              */
/* ========================================================================================== */
int s2svc_attn_fused_supported(int dtype, int T1, int T2, int dk);
int s2svc_attn_fused_fwd(int B, int H, int T1, int T2, int dk, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk,
                         int64_t kbs, const void* v, int64_t ldv, int64_t vbs, const int32_t* klen, int causal, float scale,
                         float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* attn, int ld, void* out, int64_t ldo,
                         int64_t obs, void* stream);
int s2svc_attn_fused_bwd(int B, int H, int T1, int T2, int dk, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk,
                         int64_t kbs, const void* v, int64_t ldv, int64_t vbs, const void* dout, int64_t ldo, int64_t obs,
                         const void* attn, const void* dattn, int ld, float scale, float drop_p, const uint64_t* seed_base,
                         uint64_t seed_off, void* dq, int64_t lddq, int64_t dqbs, void* dk_out, int64_t lddk, int64_t dkbs, void* dv,
                         int64_t lddv, int64_t dvbs, void* stream);

/* The same backward with the out-projection's data gradient as its prologue (attn_proj_bwd_kernel): */
/* instead of dout = dctx it reads dy (B, T1, D), the gradient of the out-projection's OUTPUT    */
/* (element [b*ybs + t*ldy + n]), and wot = W_o^T (D_in, D_out) bf16, row pitch ldw (the          */
/* optimiser's transposed shadow); a (b, h) workgroup computes its head's dctx columns with the   */
/* GEMM's instruction, K order and rounding, and dctx is never written.  D = H*dk <= 512.         */
/* s2svc_attn_proj_supported: nproj = 0 asks for this backward; nproj = 1 / 3 (Q / Q|K|V folded   */
/* into the forward) are reserved and reported unsupported.                                       */
int s2svc_attn_proj_supported(int dtype, int T1, int T2, int dk, int D, int nproj);
int s2svc_attn_proj_bwd(int B, int H, int T1, int T2, int dk, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk,
                        int64_t kbs, const void* v, int64_t ldv, int64_t vbs, const void* dy, int64_t ldy, int64_t ybs,
                        const void* wot, int64_t ldw, const void* attn, const void* dattn, int ld, float scale, float drop_p,
                        const uint64_t* seed_base, uint64_t seed_off, void* dq, int64_t lddq, int64_t dqbs, void* dk_out,
                        int64_t lddk, int64_t dkbs, void* dv, int64_t lddv, int64_t dvbs, void* stream);

/* ========================================================================================== */
/* Relative-position self-attention without the (B, H, T, 2T-1) position term in memory        */
/* (csrc/relattn.hip): bf16, T <= 256, d_k % 32 == 0, the "new" rel_shift (pos has 2T-1 rows). */
/* replaces: modules/transformer/attention.py:237-260 (rel_shift), :283-303 (q + pos_bias_u/v, */
/* matrix_ac, matrix_bd, the shift, the scaling) and :63-93 (mask, softmax, mask) forward; the */
/* backward of the same up to the gradient of the scaled scores and of matrix_bd.              */
/*   fwd: attn / pdrop (B, H, T, ld) bf16 (pdrop = the dropped copy, NULL when drop_p == 0),   */
/*        qu = q + pos_bias_u, qv = q + pos_bias_v (B, T, H*dk) for the backward GEMMs.        */
/* ========================================================================================== */
int s2svc_relattn_supported(int dtype, int T, int dk, int rel_mode);
int s2svc_relattn_fwd(int B, int H, int T, int dk, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk, int64_t kbs,
                      const void* pos, int64_t ldp, int L, const float* u, const float* v, const int32_t* klen, float scale,
                      float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* attn, void* pdrop, int ld, void* qu, void* qv,
                      void* stream);

/* ========================================================================================== */
/* Attention map of plain multi-head attention, medium sequences (csrc/attn_map.hip): bf16,   */
/* T2 <= 512 keys, d_k % 32 == 0.  replaces: modules/transformer/attention.py:63-93 (scores / */
/* sqrt(d_k), masked_fill(min), softmax, masked_fill(0), dropout) as one launch; the context   */
/* P.V stays a GEMM.  q (B, T1, .) / k (B, T2, .) views (row strides ldq / ldk, batch strides  */
/* qbs / kbs, head h at columns h * dk); klen (B) int32 or NULL; causal: keys j <= i only;     */
/* attn / pdrop (B, H, T1, ld) bf16, ld = T2 rounded up to 8, pad columns zero (pdrop = the    */
/* dropped copy, NULL when drop_p == 0); masks as s2svc_attn_softmax_fwd draws them.           */
/* ========================================================================================== */
int s2svc_attn_map_supported(int dtype, int T1, int T2, int dk);
/* 1 when the launches below can also carry the product of their finished tile with a (T2, d_k) matrix of the head (d_k in {64, 96,   */
/* 128}): forward the context ctx = (dropped map) . v (attention.py:95-111 up to the output projection), backward dq = dS . k.        */
int s2svc_attn_map_product_supported(int dk);
/* v != NULL: ctx (B, T1, .) view (row stride ldc, batch stride cbs) receives the context in the same launch. */
int s2svc_attn_map_fwd(int B, int H, int T1, int T2, int dk, const void* q, int64_t ldq, int64_t qbs, const void* k, int64_t ldk,
                       int64_t kbs, const int32_t* klen, int causal, float scale, float drop_p, const uint64_t* seed_base,
                       uint64_t seed_off, void* attn, void* pdrop, int ld, const void* v, int64_t ldv, int64_t vbs, void* ctx,
                       int64_t ldc, int64_t cbs, void* stream);
/* backward of the same up to the gradient of the scaled scores: ds = attn * (dP * mask + dattn - rowsum(attn * (dP * mask + dattn)))  */
/* * scale with dP = dctx . v^T computed on chip (replaces one batched GEMM + s2svc_attn_softmax_bwd); dctx (B, T1, .) / v (B, T2, .)  */
/* views, attn the stored map, dattn the gradient that reached the map itself (or NULL), ds (B, H, T1, ld) bf16, pad columns zero.     */
/* dbd != NULL: relative-position self-attention (attention.py:237-260 "new" rel_shift, T1 == T2): dbd (B, H, T1, ldb) bf16 receives   */
/* the gradient of matrix_bd BEFORE the shift (dbd[b,h,i,T1-1-i+j] = ds[b,h,i,j], zero elsewhere; ldb >= 2 T1 - 1, a multiple of 8).   */
/* k != NULL: dq (B, T1, .) view (row stride lddq, batch stride dqbs) receives ds . k in the same launch.                              */
int s2svc_attn_map_bwd(int B, int H, int T1, int T2, int dk, const void* dctx, int64_t ldo, int64_t obs, const void* v, int64_t ldv,
                       int64_t vbs, const void* attn, const void* dattn, float scale, float drop_p, const uint64_t* seed_base,
                       uint64_t seed_off, void* ds, int ld, void* dbd, int ldb, const void* k, int64_t ldk, int64_t kbs, void* dq,
                       int64_t lddq, int64_t dqbs, void* stream);

/* ========================================================================================== */
/* Token embedding of Transformer-TTS (models/transformer_tts.py:63-77, Embedding(idim, adim, */
/* padding_idx=0)): y[i,:] = W[idx[i],:] ; dW[v,:] = sum_{idx[i]==v} dy[i,:], dW[padding]=0     */
/* ========================================================================================== */
int s2svc_embedding_fwd(int dtype, int64_t n, int D, int V, const int64_t* idx, const float* w, void* y, void* stream);
int s2svc_embedding_bwd(int dtype, int64_t n, int D, int V, const int64_t* idx, const void* dy, int64_t padding_idx,
                        float* dw, int accumulate, void* stream);

/* ========================================================================================== */
/* Stochastic duration predictor (VITS flows), channel-last rows r=(b,t), mask = t < lens[b]   */
/* replaces: modules/duration_predictor.py:211-304, modules/vits/flow.py:18-310,               */
/* modules/vits/transform.py:17-216.  Spline / glue stages are fp32.                           */
/* ========================================================================================== */
int s2svc_mask_rows(int dtype, int B, int T, int C, const void* x, const int32_t* lens, void* y, void* stream);
/* Conv1d(1->C,k=1) + conditioning, masked: y[r,c] = mask*(a[r]*w[c] + bias[c] + g[r,c])   (flow.py:290-292) */
int s2svc_expand_fwd(int dtype, int B, int T, int C, const float* a, const float* w, const float* bias, const void* g,
                     const int32_t* lens, void* y, void* stream);
/* dg = mask*dy ; da[r] = sum_c dg[r,c]*w[c]   (dw, dbias: s2svc_colreduce mode 5 over dg with v = a) */
int s2svc_expand_bwd(int dtype, int B, int T, int C, const void* dy, const float* w, const int32_t* lens, void* dg, float* da,
                     void* stream);
/* y = mask*(res + dropout(act(LayerNorm(x))))   (one DDS half-layer, flow.py:148-190); res / lens optional, D <= 1024 */
int s2svc_ln_act_fwd(int dtype, int rows, int D, int T, const void* x, const float* gamma, const float* beta, float eps, int act,
                     const void* res, const int32_t* lens, float drop_p, const uint64_t* seed_base, uint64_t seed_off, void* y,
                     float* mean, float* rstd, void* stream);
/* the first half of a DDS layer in one launch (fp32): u = depthwise Conv1d(x; dw_w (D, ks), dw_b, dilation dil, zero padding inside
   the T frames of an utterance) -- flow.py:137-146 -- written out for the backward pass, y = act(LayerNorm(u)); D <= 512, ks odd */
int s2svc_dw_ln_act_fwd(int B, int T, int D, int ks, int dil, const float* x, const float* dw_w, const float* dw_b,
                        const float* gamma, const float* beta, float eps, int act, float* u, float* y, float* mean, float* rstd,
                        void* stream);
/* du = gradient at the LayerNorm output (feeds dgamma/dbeta via colreduce mode 1), dx = LN input grad, dres = mask*dy */
int s2svc_ln_act_bwd(int dtype, int rows, int D, int T, const void* dy, const void* x, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, int act, const int32_t* lens, float drop_p,
                     const uint64_t* seed_base, uint64_t seed_off, void* du, void* dx, void* dres, void* stream);

/* rational-quadratic spline coupling with linear tails; h (rows, 3*bins-1); lad accumulates when asked (transform.py:96-216) */
int s2svc_rq_spline_fwd(int B, int T, int bins, const float* x, const float* h, float hscale, float bound, const int32_t* lens,
                        int inverse, float* out, float* lad, int lad_accumulate, void* stream);
/* g_lad: (B) gradient shared by all rows of an utterance (the log-dets are summed over t) */
int s2svc_rq_spline_bwd(int B, int T, int bins, const float* x, const float* h, float hscale, float bound, const int32_t* lens,
                        const float* g_out, const float* g_lad, float* dx, float* dh, void* stream);
/* glue: noise -> first affine flow | dequantise + log flow + affine | per-utterance NLL (duration_predictor.py:239-280) */
int s2svc_sdp_head_fwd(int B, int T, const float* noise, const int32_t* lens, const float* m, const float* logs, float* z0,
                       float* z1, void* stream);
int s2svc_sdp_head_bwd(int B, int T, const float* noise, const int32_t* lens, const float* logs, const float* dz0,
                       const float* dz1, float* part, void* stream);
int s2svc_sdp_mid_fwd(int B, int T, const float* zu, const float* z1, const float* w, const int32_t* lens, const float* m,
                      const float* logs, float* y0, float* y1, float* lz, void* stream);
int s2svc_sdp_mid_bwd(int B, int T, const float* zu, const float* z1, const float* w, const int32_t* lens, const float* logs,
                      const float* dy0, const float* dy1, const float* dlz, float* dzu, float* dz1, float* part, void* stream);
int s2svc_sdp_tail_fwd(int B, int T, const float* noise, const int32_t* lens, const float* zu, const float* lz,
                       const float* lad_q, const float* lad_p, const float* af, const float* bf, const float* logs_q,
                       const float* logs_p, float* out, int normalize /* 1: / sum_b min(lens[b], T), aas_vc.py:403 */, void* stream);
int s2svc_sdp_tail_bwd(int B, int T, const float* g, const int32_t* lens, const float* zu, const float* af, const float* bf,
                       float* d_af, float* d_bf, float* d_lz, float* d_zu, float* neg_g, float* part, int normalize, void* stream);
/* inference read-out: dur = ceil(exp((a - m0)*exp(-logs0)))*mask   (duration_predictor.py:300-304) */
int s2svc_sdp_inverse_out(int B, int T, const float* a, const int32_t* lens, const float* m, const float* logs, float* dur,
                          void* stream);

/* ========================================================================================== */
/* Autoregressive decode step (static K/V cache, device-resident step index, device stop test) */
/* replaces: models/vtn.py:344-389 / models/transformer_tts.py:268-321 (generation loop),      */
/* modules/transformer/decoder.py:239-273 (forward_one_step), decoder_layer.py:85-132 (cache). */
/* `pos` is one device int32 (0-based position of the frame being generated); every kernel of */
/* a step reads it, s2svc_decode_advance bumps it: one captured hipGraph serves all steps.    */
/* ========================================================================================== */
/* y[b,:] = x[b,:]*xscale + alpha*pe[pos,:]   (embedding.py:73-88 / :115-125 for one position) */
int s2svc_decode_posenc(int dtype, int B, int D, const void* x, float xscale, const float* alpha, const float* pe,
                        const int32_t* pos, void* y, void* stream);
/* one query row per (utterance, head) against a K/V cache (B, Tk, .) with time stride ldt and batch stride cbs.   */
/* knew/vnew != NULL (self-attention): the row is first appended at position *pos, keys 0..*pos are attended;      */
/* else (source attention) keys 0..klen[b]-1.  att != NULL: probabilities (zeros past the valid keys) are stored   */
/* at att[b*att_bs + h*att_hs + *pos*att_ps + j], j < Tk  (vtn.py:364-375 collects src_attn.attn[0,:,-1]).          */
int s2svc_decode_attn(int dtype, int B, int H, int dk, const void* q, int64_t ldq, void* kcache, void* vcache,
                      int64_t ldt, int64_t cbs, const void* knew, const void* vnew, int64_t ldn, const int32_t* pos,
                      const int32_t* klen, int Tk, float scale, void* ctx, int64_t ldo, float* att, int64_t att_bs,
                      int64_t att_hs, int64_t att_ps, void* stream);
/* outs[b, pos*r+i, :] = feat[b, i, :]; probs = sigmoid(logit); prev[b,:] = last frame; stop test vtn.py:378-381 */
int s2svc_decode_emit(int dtype, int B, int r, int odim, const void* feat, const void* logit, float threshold,
                      const int32_t* minlen, const int32_t* maxlen, const int32_t* pos, float* outs, int64_t outs_bs,
                      float* probs, int64_t probs_bs, void* prev, int32_t* stop_at, void* stream);
int s2svc_decode_advance(int32_t* pos, uint64_t* seed_base, uint64_t seed_stride, void* stream);
/* LayerNorm -> Linear of a decode step, one launch: C[M <= 64, N] = act(LN(A)[M, K] . B[N, K]^T + bias) [dropout] (+ res);
   `desc` carries A (the pre-LayerNorm rows), B, C and the epilogue fields of s2svc_gemm (dense K-contiguous operands,
   unbatched, unsplit); gamma / beta / eps: the LayerNorm (both NULL: plain skinny linear); y_out != NULL: LN(A) is also
   written there (row stride ldy) -- the residual input of a post-LN layer (decoder_layer.py:104-127).
   Replaces one LayerNorm launch + one Linear launch per projection of decoder.py:239-273. */
/* 1 if s2svc_decode_ln_linear takes an (M x K) input of this dtype (else: s2svc_layernorm_fwd + s2svc_gemm) */
int s2svc_decode_ln_linear_supported(int dtype, int M, int K);
int s2svc_decode_ln_linear(const s2svc_gemm_desc* desc /* host */, const float* gamma, const float* beta, float eps, void* y_out,
                           int64_t ldy, void* stream);
/* Round 6 (csrc/decode_fused.hip): s2svc_decode_emit on ONE packed feat_out | prob_out projection (feat / logit rows with stride ldf)
   + s2svc_decode_advance by the last workgroup to finish (`ticket`: one zero-initialised device uint32, zero again afterwards)
   + pe_next != NULL: pe_next[0 .. D) = alpha * pe[(*pos + 1) * D + .] in `dtype` -- the positional-encoding row of the NEXT position,
   which the input Linear of the next step adds as a residual with row stride 0 (embedding.py:115-125; no s2svc_decode_posenc launch). */
int s2svc_decode_emit_advance(int dtype, int B, int r, int odim, const void* feat, const void* logit, int64_t ldf, float threshold,
                              const int32_t* minlen, const int32_t* maxlen, int32_t* pos, float* outs, int64_t outs_bs, float* probs,
                              int64_t probs_bs, void* prev, int32_t* stop_at, uint64_t* seed_base, uint64_t seed_stride,
                              uint32_t* ticket, const float* pe, const float* alpha, int D, int pe_rows, void* pe_next, void* stream);

/* ========================================================================================== */
/* Optimiser: grad-norm -> clip -> WarmupLR -> Adam (+ bf16 shadow) over one flat buffer       */
/* replaces: trainers/ar_vc.py:99-107 (clip_grad_norm_, Adam.step, scheduler.step),            */
/* schedulers/warmup_lr.py:54-61.  state: 4 device floats {step, lr, grad_norm, clip_coef}.    */
/* A refused call (rc -1: bad arguments, buffers not 16-byte aligned) launches nothing and    */
/* leaves state, params and both moments as they were.                                        */
/* ========================================================================================== */
int s2svc_adam_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                    float beta1, float beta2, float eps, float max_norm, float base_lr, float warmup_steps,
                    double* partial, float* state, void* stream);

/* dst[c, r] = src[r, c] (bf16) for every 64x64 tile listed in `tiles` (device, 4 x int64 per tile: src offset of  */
/* the matrix, dst offset, rows<<32|cols, tile index): keeps W^T beside the bf16 weight shadow so that the data-  */
/* gradient GEMMs read K-contiguous operands.                                                                   */
int s2svc_transpose_tiles(int64_t ntiles, const int64_t* tiles, const void* src, void* dst, void* stream);

/* ========================================================================================== */
/* STFT -> log-mel glue (the two contractions use s2svc_gemm)                                  */
/* replaces: bin/preprocess.py:63-92 (librosa.stft reflect padding, abs, max(eps,.), log10)    */
/* and optionally bin/normalize.py:172-193 ((x-mean)/scale fused into the log kernel).         */
/* ========================================================================================== */
int s2svc_reflect_pad(int64_t n, int pad, const float* x, float* y, void* stream);
int s2svc_magnitude(int64_t frames, int nb, const float* z, float* spc, void* stream);
int s2svc_log_clamp(int64_t n, int D, const float* x, float eps, float inv_log_base, const float* mean,
                    const float* inv_scale, float* y, void* stream);

/* Batched form: B utterances per launch, wav batch -> normalised zero-padded (B, Tmax, n_mels) log-mel batch -- what
   bin/preprocess.py:200-310 (one utterance at a time), bin/normalize.py:172-193 and the collater's padding
   (collaters/ar_vc.py:42-45) produce in three passes over HDF5 files.
     s2svc_reflect_pad_batch: x (B, Nmax) zero-padded waveforms, nlen (B) sample counts -> y (B, ld), ld >= Nmax + 2*pad:
         row b = reflect-padded utterance b followed by zeros (frames past the utterance then transform zeros);
     [one batched s2svc_gemm: A = y with row stride `hop` and batch stride ld, B = windowed DFT basis -> z (B, Tmax, 2*nb)]
     s2svc_mel_log_batch: z -> out (B, Tmax, nmel): magnitude, mel projection over each filter's bins [lo, hi) only,
         max(eps, .), log, optional (x - mean) * inv_scale; frames t >= frames[b] are written as zeros.
     s2svc_ragged_to_padded: ragged feature rows (concatenated utterances, row offsets (B + 1) int64) -> (B, Tmax, D)
         zero-padded batch (+ optional normalisation, + optional stop labels (B, Tmax): 1 from the last valid frame on). */
int s2svc_reflect_pad_batch(int B, int64_t Nmax, int pad, int64_t ld, const float* x, const int32_t* nlen, float* y, void* stream);
/* The same batch in ONE launch with the FFT in LDS (csrc/stft_fft.hip; n_fft in {512, 1024, 2048}): one wavefront per frame --
   windowed load with the reflect padding as index arithmetic, N/2-point complex radix-4 Stockham FFT of the even/odd packed
   frame, unpack, magnitude, sparse mel projection, clamp, log, normalisation, zero rows for the padding frames.
     tables (16-byte aligned, fp32, zero-filled to whole 16-byte vectors): w_half [n_fft/2] complex exp(-2 pi i m / (n_fft/2)) |
     w_full [n_fft/2 + 1] complex exp(-2 pi i k / n_fft) | win [n_fft] | melw [melw_n rounded up to even];
     melw: the non-zero weights of filter m are melw[mel_off[m] .. mel_off[m] + mel_hi[m] - mel_lo[m]) for bins [mel_lo, mel_hi);
     mel_maxw = the widest filter (bins); the list (melw_n values) ends with a zero tail of at least mel_maxw + 1 values. */
int s2svc_stft_logmel_fft_supported(int n_fft, int nmel, int melw_n);
int s2svc_stft_logmel_fft(int B, int64_t Nmax, int Tmax, int n_fft, int hop, int nmel, const float* x, const int32_t* nlen,
                          const int32_t* frames, const float* tables, const int32_t* mel_lo, const int32_t* mel_hi, const int32_t* mel_off, int melw_n, int mel_maxw,
                          float eps, float inv_log_base, const float* mean, const float* inv_scale, float* out, void* stream);

/* n_fft = 1024 and triangular mel filters (every bin has at most two non-zero weights, in neighbouring filters; n_mels <= 128): the
   512-point FFT as three passes of in-register 8-point DFTs, per-lane tables in registers, mel projection by segments.
     tables: the packed table of s2svc_stft_logmel_fft (w_half | w_full | win are read);
     seg_lo / seg_len [nmel]: the contiguous bin range whose HIGHEST filter is m;  wud [513][2]: weight of that filter and of the
     one below it at bin k;  mel[m] = sum_{k in seg m} wud[k][0] |X[k]| + sum_{k in seg m+1} wud[k][1] |X[k]|. */
int s2svc_stft_logmel_fft8(int B, int64_t Nmax, int Tmax, int hop, int nmel, const float* x, const int32_t* nlen, const int32_t* frames,
                           const float* tables, const int32_t* seg_lo, const int32_t* seg_len, const float* wud, float eps,
                           float inv_log_base, const float* mean, const float* inv_scale, float* out, void* stream);

int s2svc_mel_log_batch(int B, int Tmax, int nb, int nmel, const float* z, const int32_t* frames, const float* melb,
                        const int32_t* lo, const int32_t* hi, float eps, float inv_log_base, const float* mean,
                        const float* inv_scale, float* out, void* stream);
int s2svc_ragged_to_padded(int B, int Tmax, int D, const float* ragged, const int64_t* offsets, const float* mean,
                           const float* inv_scale, float* out, float* labels, void* stream);

/* ========================================================================================== */
/* HiFi-GAN generator, inference (csrc/hifigan.hip).  Channel-last activations (B, T, C) in    */
/* `dtype`; absent rows: frames t >= vlens[b] * vmul (vlens counts MEL frames, vmul = the      */
/* product of the upsampling factors so far; vlens = NULL: every frame present) are read as    */
/* zero by every tap and written as zero.  No element-wise launches: leaky_relu is applied to  */
/* the A operand on its way into the MFMA (slope 0 = none), everything else in the epilogue.   */
/* replaces: urhythmic/vocoder.py:87-106 (HifiganGenerator.forward), :195-202 (ResBlock).      */
/* ========================================================================================== */
/* input channels per reduction step: the operands below pad C_in up to this multiple */
int s2svc_hifigan_cin_padded(int C);
/* Dilated Conv1d, k odd <= 11, dil <= 5, padding (k-1)/2*dil, 1 <= C_in, C_out <= 512 (vocoder.py:56-58 conv_pre, :125-193 convs1 /
   convs2):  v = conv(leaky_relu(x, slope)) + bias (+ res);  out = (accumulate ? out : 0) + scale * v;  optional tanh.
   w_op [C_out][k * Cinp] (s2svc_hifigan_fold mode 0).  res / out (B, T, C_out); out may be res. */
int s2svc_hifigan_conv1d(int dtype, int B, int T, int Cin, int Cout, int k, int dil, const void* x, const void* w_op, const float* bias,
                         float slope, const void* res, int accumulate, float scale, int act_tanh, void* out, const int32_t* vlens,
                         int vmul, void* stream);
/* ConvTranspose1d, stride u, kernel k, padding (k-u)/2 ((k-u) even, k >= u) as one GEMM without scatter or col2im (vocoder.py:61-73
   ups[i], with the leaky_relu of :94 in front): rows (b, i), i < T_in + ceil(pad/u), columns (p, o), reduction ceil(k/u) * Cinp,
   column p of row i is stored at frame t = u*i + p - pad of out (B, u*T_in, C_out).  w_op: s2svc_hifigan_fold mode 1.
   vmul counts the INPUT frames per mel frame. */
int s2svc_hifigan_tconv1d(int dtype, int B, int Tin, int Cin, int Cout, int k, int u, const void* x, const void* w_op, const float* bias,
                          float slope, void* out, const int32_t* vlens, int vmul, void* stream);
/* Output convolution C -> 1 (vocoder.py:103-105: leaky_relu (torch's default slope 0.01), conv_post, tanh), one lane per sample:
   y (B, T) fp32; y_pre (or NULL) receives the value before tanh; w [k][C] fp32 (s2svc_hifigan_fold mode 2). */
int s2svc_hifigan_conv_out(int dtype, int B, int T, int C, int k, const void* x, const float* w, const float* bias, float slope,
                           int act_tanh, float* y, float* y_pre, const int32_t* vlens, int vmul, void* stream);
/* Input launch: x element (b, t, c) at b*sb + t*st + c*sc (any strides: the reference's (B, C, N) or the collaters' (B, N, C)) ->
   out (B, T, C) in out_dtype = a[c] * x + b[c] (a, b fp32 [C] or NULL: the two normalisations of vocoder/vocoder.py:50-55 as one
   map); frames t >= vlens[b] are written as zero whatever the input holds. */
int s2svc_hifigan_input(int in_dtype, int out_dtype, int B, int T, int C, const void* x, int64_t sb, int64_t st, int64_t sc,
                        const float* a, const float* b, void* out, const int32_t* vlens, void* stream);
/* Weight-norm fold (torch.nn.utils.weight_norm at vocoder.py:56-85, 125-193): w = v * (g / ||v||), norm over all dims but 0, v (D0, D1, k)
   fp32; g = NULL: v is the weight.  Writes w32 (or NULL) in v's layout and the operand w_op (or NULL; ZERO-FILLED by the caller):
   mode 0 Conv1d (O, C, k) -> [o][j*Cinp + c];  mode 1 ConvTranspose1d (C, O, k) -> [p*O + o][n*Cinp + c] = w[c, o, p + u*n];
   mode 2 output convolution (1, C, k) -> fp32 [j*C + c]. */
int s2svc_hifigan_fold(int mode, int D0, int D1, int k, int u, const float* g, const float* v, float* w32, int op_dtype, void* w_op,
                       void* stream);

/* ========================================================================================== */
/* HiFi-GAN generator, backward with respect to the parameters (csrc/hifigan_bwd.hip).  The    */
/* same channel-last tensors in `dtype`, no absent rows (training batches are not ragged).     */
/* Masks are the forward's RAW layer inputs: lrelu'(m, s) = 1 for m > 0, s otherwise.  Every   */
/* sum runs in an order fixed by the shapes: no atomics, two passes give the same bits.        */
/* replaces: loss.backward() through urhythmic/vocoder.py:87-106, :195-202                     */
/* (urhythmic_fine_tune_vocoder.py:191-222).                                                   */
/* ========================================================================================== */
/* Operand of the data gradient from the folded fp32 weight w32 (D0, D1, k); w_opT is ZERO-FILLED by the caller.
   mode 0 Conv1d (O, C, k) -> [c][j*Op + o] = w[o, c, k-1-j], Op = O padded;  mode 1 ConvTranspose1d (C, O, k) ->
   [c][n*Kp + p*O + o] = w[c, o, p + u*n], Kp = u*O padded (s2svc_hifigan_cin_padded). */
int s2svc_hifigan_fold_bwd(int mode, int D0, int D1, int k, int u, const float* w32, int op_dtype, void* w_opT, void* stream);
/* Data gradient of s2svc_hifigan_conv1d: dx (B, T, C_in) = (accumulate ? dx : 0) + scale * (lrelu'(mask_src, slope) * conv(dy, w
   flipped and transposed) (+ res)); dy (B, T, C_out); mask_src / res (B, T, C_in) or NULL. */
int s2svc_hifigan_conv1d_dgrad(int dtype, int B, int T, int Cin, int Cout, int k, int dil, const void* dy, const void* w_opT,
                               const void* mask_src, float slope, const void* res, int accumulate, float scale, void* dx, void* stream);
/* Data gradient of s2svc_hifigan_tconv1d: dy (B, u*T_in, C_out) is read as the forward's GEMM rows (i, (p, o)) at a flat offset of
   -pad*C_out elements, zero outside the utterance; dx (B, T_in, C_in) = scale * lrelu'(mask_src, slope) * sum_n dy'[i + n] . op[n]. */
int s2svc_hifigan_tconv1d_dgrad(int dtype, int B, int Tin, int Cin, int Cout, int k, int u, const void* dy, const void* w_opT,
                                const void* mask_src, float slope, float scale, void* dx, void* stream);
/* Weight and bias gradient partials.  kind 0 Conv1d: dy (B, T, C_out), x (B, T, C_in), dil_or_u = dilation; kind 1 ConvTranspose1d:
   dy (B, u*T, C_out), x (B, T, C_in), dil_or_u = stride.  The rows of an utterance (T, or T + ceil(pad/u)) are cut into chunks of
   `chunk` frames (a multiple of 32); chunk q of utterance b writes wpart[b*ncpu + q][Na][ntaps][C_in] = sum over its rows of
   dy'[i][m] * leaky_relu(x, slope)[i + offset(tap)][c] and bpart[b*ncpu + q][Na] = the column sums of dy'; Na = C_out or u*C_out,
   ntaps = k or ceil(k/u) (<= 12).  A halo crosses a chunk edge inside the utterance and reads zero past the utterance's ends. */
int s2svc_hifigan_wgrad(int dtype, int kind, int B, int T, int Cin, int Cout, int k, int dil_or_u, int chunk, const void* dy,
                        const void* x, float slope, float* wpart, float* bpart, void* stream);
/* Sum of nparts partials in ascending order -> the parameter's layout (D0, D1, k) (modes as s2svc_hifigan_fold; mode 1 drops the
   slots p + u*n >= k; mode 2 partials are [nparts][k][C] / [nparts]), then the weight-norm backward over dim 0 when g is given:
   grad_g = sum(dw * v) / ||v||, grad_w (= grad_v) = (g / ||v||) dw - (g sum(dw * v) / ||v||^3) v; g = NULL: grad_w = dw.
   grad_bias (or NULL) = the summed bias partials. */
int s2svc_hifigan_wgrad_finish(int mode, int D0, int D1, int k, int u, int nparts, const float* wpart, const float* bpart, const float* g,
                               const float* v, float* grad_w, float* grad_g, float* grad_bias, void* stream);
/* Backward of s2svc_hifigan_conv_out with tanh: dpre = dy * (1 - y^2); dx (B, T, C) = scale * lrelu'(x, slope) * the C -> 1 data
   gradient; wpart [B * ceil(T/chunk)][k][C] and bpart [B * ceil(T/chunk)]: partials per chunk of frames (chunk = 256, the workgroup's
   share; the caller states it so that both sides size the partials alike).  y, dy (B, T) fp32. */
int s2svc_hifigan_conv_out_bwd(int dtype, int B, int T, int C, int k, int chunk, const void* x, const float* w, const float* y, const float* dy,
                               float slope, float scale, void* dx, float* wpart, float* bpart, void* stream);

/* ========================================================================================== */
/* HiFi-GAN multi-period discriminator, forward and backward, fp32 (csrc/hifigan_disc.hip).    */
/* One PeriodDiscriminator of period p folds x (B, 1, T) into (B, 1, L0, p), L0 = ceil(T / p)  */
/* (reflect pad on the right), and convolves along L only.  Activations are channel-last       */
/* (B, L, p, C) and hold the POST-activation values (they are the features the caller gets);   */
/* a row is (b, l, w).  A convolution (k = 5, padding 2, stride s) maps L to (L - 1) / s + 1;  */
/* rows outside [0, L) of the same (b, w) sequence are zero.  leaky_relu'(m) = 1 for m > 0,    */
/* slope otherwise, taken from the stored output.  Weight norm: s2svc_hifigan_fold mode 0 / 2  */
/* on the (O, C, k) view of weight_v, s2svc_hifigan_fold_bwd mode 0, and                       */
/* s2svc_hifigan_wgrad_finish mode 0 / 2 over the partials below.  No atomics: every sum runs  */
/* in an order fixed by the shapes.                                                            */
/* replaces: urhythmic/vocoder.py:211-327 (PeriodDiscriminator, MultiPeriodDiscriminator) and  */
/* loss.backward() through them (urhythmic_fine_tune_vocoder.py:191-222).                      */
/* ========================================================================================== */
/* Input layer 1 -> 32, k = 5, stride 3: out (B, L1, p, 32) = leaky_relu(conv(x') + bias), x' = x (B, T) reflect-padded to L0 * p
   samples and viewed (L0, p) -- both by index arithmetic, no padded copy.  w32 [32][5] (s2svc_hifigan_fold's w32 of (32, 1, 5)).
   replaces: urhythmic/vocoder.py:278-287 (F.pad reflect, view, convs[0], leaky_relu) */
int s2svc_hifigan_disc_input(int B, int T, int p, const float* x, const float* w32, const float* bias, float slope, float* out,
                             void* stream);
/* Strided convolution as an implicit GEMM on MFMA: x (B, L, p, C_in) -> out (B, (L - 1) / stride + 1, p, C_out) =
   leaky_relu(conv + bias); stride 1 or 3, C_in a multiple of 16, C_out of 4; w_op [C_out][5 * Cinp] (s2svc_hifigan_fold mode 0).
   replaces: urhythmic/vocoder.py:285-288 (convs[1..4], leaky_relu) */
int s2svc_hifigan_disc_conv(int B, int L, int p, int Cin, int Cout, int stride, const float* x, const float* w_op, const float* bias,
                            float slope, float* out, void* stream);
/* conv_post C -> 1, k = 3, padding 1, no activation: y (B, L * p) in (l, w) order; w [3][C] (s2svc_hifigan_fold mode 2).
   replaces: urhythmic/vocoder.py:289-291 (conv_post, flatten) */
int s2svc_hifigan_disc_post(int B, int L, int p, int C, const float* x, const float* w, const float* bias, float* y, void* stream);
/* Backward of s2svc_hifigan_disc_post: d = dy1 + dy2 (each (B, L * p) or NULL: the gradients of the score and of the last feature);
   dx (B, L, p, C) = leaky_relu'(x) * (add + the C -> 1 data gradient), add (B, L, p, C) or NULL = the gradient of the feature x itself;
   wpart [chunks][3][C], bpart [chunks] over chunks of 256 rows of B * L * p.
   replaces: autograd of urhythmic/vocoder.py:287-291 */
int s2svc_hifigan_disc_post_bwd(int B, int L, int p, int C, const float* x, const float* w, const float* dy1, const float* dy2,
                                const float* add, float slope, float* dx, float* wpart, float* bpart, void* stream);
/* Weight / bias gradient partials of s2svc_hifigan_disc_conv: dy (B, Lo, p, C_out) = the gradient of the PRE-activation, x (B, L, p, C_in)
   the layer's input; chunk q covers rows [256 q, 256 q + 256) of B * Lo * p: wpart [chunks][C_out][5][C_in], bpart [chunks][C_out].
   replaces: autograd of urhythmic/vocoder.py:285-288 (weight and bias gradients of convs[1..4]) */
int s2svc_hifigan_disc_wgrad(int B, int L, int p, int Cin, int Cout, int stride, const float* dy, const float* x, float* wpart,
                             float* bpart, void* stream);
/* Data gradient of s2svc_hifigan_disc_conv: dy (B, Lo, p, C_out) -> dx (B, L, p, C_in) = leaky_relu'(mask_src) * (add + conv^T(dy)),
   mask_src / add (B, L, p, C_in) or NULL: the stored output of the layer below and the gradient of that feature.  Stride 3 is
   phase-decomposed: row l receives only the taps j = l + 2 (mod 3).  w_opT: s2svc_hifigan_fold_bwd mode 0; C_out a multiple of 16.
   replaces: autograd of urhythmic/vocoder.py:285-288 (data gradient of convs[1..4], leaky_relu backward) */
int s2svc_hifigan_disc_dgrad(int B, int L, int p, int Cin, int Cout, int stride, const float* dy, const float* w_opT, const float* mask_src,
                             const float* add, float slope, float* dx, void* stream);
/* Weight / bias partials of the input layer: dy (B, L1, p, 32), x (B, T) -> wpart [chunks][32][5], bpart [chunks][32], chunks =
   ceil(B * L1 * p / 256).  replaces: autograd of urhythmic/vocoder.py:278-287 (gradients of convs[0]) */
int s2svc_hifigan_disc_input_wgrad(int B, int T, int p, const float* dy, const float* x, float* wpart, float* bpart, void* stream);
/* dx (B, T) of the input layer: a gather -- sample t collects its own padded position and, where the reflect pad copied it, its
   mirror image 2 (T - 1) - t.  replaces: autograd of urhythmic/vocoder.py:278-287 (F.pad reflect / view / convs[0] backward) */
int s2svc_hifigan_disc_input_dgrad(int B, int T, int p, const float* dy, const float* w32, float* dx, void* stream);

/* ========================================================================================== */
/* HiFi-GAN multi-scale discriminator, forward and backward, fp32 (csrc/hifigan_msd.hip).      */
/* Three ScaleDiscriminators see x (B, 1, T), pool(x) and pool(pool(x)).  Activations are      */
/* channel-last (B, L, C) and hold the POST-activation values (the features the caller gets).  */
/* A convolution (k taps, padding (k - 1) / 2, stride s) maps L to (L - 1) / s + 1; rows       */
/* outside [0, L) of an utterance are zero and a column tile lies inside one group.            */
/* leaky_relu'(m) = 1 for m > 0, slope otherwise, taken from the stored output.  Weight norm   */
/* (scales 1, 2): s2svc_hifigan_fold mode 0 / 2 on weight_v (O, C / groups, k) and             */
/* s2svc_hifigan_wgrad_finish mode 0 / 2 over the partials.  Spectral norm (scale 0): the      */
/* s2svc_hifigan_msd_sn_* launches and the same fold / finish with g = NULL.  Layer 6          */
/* (1024 -> 1024, 5 taps) and conv_post are s2svc_hifigan_disc_conv / _dgrad / _wgrad / _post  */
/* / _post_bwd at p = 1.  No atomics: every sum runs in an order fixed by the shapes.          */
/* replaces: urhythmic/vocoder.py:330-402 (ScaleDiscriminator, MultiScaleDiscriminator) and    */
/* loss.backward() through them (urhythmic_fine_tune_vocoder.py:191-222).                      */
/* ========================================================================================== */
/* AvgPool1d(4, 2, padding 2), the padding counted: y (B, T / 2 + 1), y[t] = 0.25 * sum_{j < 4} x[2 t - 2 + j], zeros outside x (B, T).
   replaces: urhythmic/vocoder.py:380-398 (meanpools) */
int s2svc_hifigan_msd_pool(int B, int T, const float* x, float* y, void* stream);
/* Its adjoint: dx (B, T) from dy (B, T / 2 + 1), a gather with one lane per sample.
   replaces: autograd of urhythmic/vocoder.py:380-398 */
int s2svc_hifigan_msd_pool_bwd(int B, int T, const float* dy, float* dx, void* stream);
/* Input layer 1 -> 128, k = 15, padding 7: out (B, T, 128) = leaky_relu(conv(x) + bias), x (B, T); w32 [128][15].
   replaces: urhythmic/vocoder.py:338, 358-361 (convs[0], leaky_relu) */
int s2svc_hifigan_msd_input(int B, int T, const float* x, const float* w32, const float* bias, float slope, float* out, void* stream);
/* Weight / bias partials of the input layer: dy (B, T, 128), x (B, T) -> wpart [chunks][128][15], bpart [chunks][128], chunks =
   ceil(B * T / 256).  replaces: autograd of urhythmic/vocoder.py:338 (gradients of convs[0]) */
int s2svc_hifigan_msd_input_wgrad(int B, int T, const float* dy, const float* x, float* wpart, float* bpart, void* stream);
/* dx (B, T) of the input layer: sample t gathers dy[t + 7 - j] . w[:, j] over the 15 taps, one wavefront per sample.
   replaces: autograd of urhythmic/vocoder.py:338 (data gradient of convs[0]) */
int s2svc_hifigan_msd_input_dgrad(int B, int T, const float* dy, const float* w32, float* dx, void* stream);
/* Grouped strided convolution, k = 41, padding 20, as an implicit GEMM on MFMA: x (B, L, C_in) -> out (B, (L - 1) / stride + 1, C_out)
   = leaky_relu(conv + bias); stride 1, 2 or 4; C_in / groups and C_out / groups multiples of 4, at most 64.
   w_op [C_out][41 * Cgp]: s2svc_hifigan_fold mode 0 of the weight (C_out, C_in / groups, 41), Cgp = C_in / groups padded to 32.
   replaces: urhythmic/vocoder.py:339-343, 358-361 (convs[1..5], leaky_relu) */
int s2svc_hifigan_msd_gconv(int B, int L, int Cin, int Cout, int groups, int stride, const float* x, const float* w_op, const float* bias,
                            float slope, float* out, void* stream);
/* Operand of the data gradient from the folded weight w32 (C_out, C_in / groups, 41): w_opT [C_in][41 * Ogp],
   [(g, c)][j * Ogp + o] = w32[g * Og + o][c][j], Og = C_out / groups, Ogp = Og padded to 32 (the padding is written as zero).
   replaces: autograd of urhythmic/vocoder.py:339-343 (the transposed weight of the data gradient) */
int s2svc_hifigan_msd_fold_bwd(int Cin, int Cout, int groups, const float* w32, float* w_opT, void* stream);
/* Data gradient of s2svc_hifigan_msd_gconv: dy (B, Lo, C_out) -> dx (B, L, C_in) = leaky_relu'(mask_src) * (add + conv^T(dy)),
   mask_src / add (B, L, C_in) or NULL: the stored output of the layer below and the gradient of that feature.  Phase-decomposed:
   row l receives only the taps j = l + 20 (mod stride), one grid plane per phase.
   replaces: autograd of urhythmic/vocoder.py:339-343 (data gradient of convs[1..5], leaky_relu backward) */
int s2svc_hifigan_msd_gconv_dgrad(int B, int L, int Cin, int Cout, int groups, int stride, const float* dy, const float* w_opT,
                                  const float* mask_src, const float* add, float slope, float* dx, void* stream);
/* Rows per partial of s2svc_hifigan_msd_gconv_wgrad for Lo output rows per utterance: max(256, 32 * ceil(Lo / 256)) -- at most
   eight partials per utterance and never fewer than one: at 8 x 8320 samples 43 MB for layers 1 and 4, 86 MB for layer 5
   (8 utterances x 10.7 MB, one chunk each), which the finish launch streams.
   replaces: nothing (the sizing rule both sides of the ABI share) */
int s2svc_hifigan_msd_gconv_chunk(int Lo);
/* Weight / bias gradient partials of s2svc_hifigan_msd_gconv: dy (B, Lo, C_out) = the gradient of the PRE-activation, x (B, L, C_in)
   the layer's input; every utterance is cut on its own into ceil(Lo / chunk) chunks of `chunk` output rows
   (= s2svc_hifigan_msd_gconv_chunk(Lo)): wpart [B * chunks][C_out][41][C_in / groups], bpart [B * chunks][C_out]; summed by
   s2svc_hifigan_wgrad_finish mode 0 with D1 = C_in / groups, k = 41.
   replaces: autograd of urhythmic/vocoder.py:339-343 (weight and bias gradients of convs[1..5]) */
int s2svc_hifigan_msd_gconv_wgrad(int B, int L, int Cin, int Cout, int groups, int stride, int chunk, const float* dy, const float* x,
                                  float* wpart, float* bpart, void* stream);
/* Spectral norm, W (O, K) = weight_orig viewed from dim 0.  iterate: v = W^T u / max(|W^T u|, eps), u = W v / max(|W v|, eps), both in
   place; then sigma[0] = u . (W v) on the device.  iterate = 0 leaves u, v untouched.  Norms and dot products in double; ws: K + O doubles.
   replaces: torch.nn.utils.spectral_norm's compute_weight as urhythmic/vocoder.py:335-347 uses it (one power iteration, eps 1e-12) */
int s2svc_hifigan_msd_sn_power(int O, int K, int iterate, float eps, const float* W, float* u, float* v, float* sigma, double* ws,
                               void* stream);
/* w = W / sigma[0], n values (the weight the convolutions of the spectrally normed scale use).
   replaces: torch.nn.utils.spectral_norm's weight = weight_orig / sigma */
int s2svc_hifigan_msd_sn_scale(int64_t n, const float* W, const float* sigma, float* w, void* stream);
/* Backward of the division with u, v constant: grad (O, K) = dW / sigma - (sum(dW o W) / sigma^2) u v^T, dW = the gradient of
   W / sigma (the summed partials); the sum in double; ws: O doubles.
   replaces: autograd through torch.nn.utils.spectral_norm (urhythmic/vocoder.py:335-347) */
int s2svc_hifigan_msd_sn_finish(int O, int K, const float* dW, const float* W, const float* u, const float* v, const float* sigma,
                                float* grad, double* ws, void* stream);

/* ========================================================================================== */
/* Griffin-Lim phase reconstruction, fp32 (csrc/griffin_lim.hip): librosa.griffinlim with      */
/* init="random" as vocoder/griffin_lim.py:53-106 calls it, for a batch with per-row lengths   */
/* in 2 n_iter + 3 launches.  Buffers: S (B, Tmax, bins) fp32, X / Rprev (B, Tmax, bins)       */
/* complex (re, im interleaved), frames (B, Tmax, n_fft) fp32, bins = n_fft / 2 + 1.  Absent   */
/* rows: frames t >= lens[b] (lens = NULL: every frame present) enter no sum and are never     */
/* read; prepare writes their S / X / Rprev as zero.  A row with fewer than two frames has no  */
/* samples and is absent as a whole.  `tables` (8-byte aligned fp32): exp(-2 pi i m / (N/2))   */
/* [N/2] complex | exp(-2 pi i k / N) [N/2 + 1] complex | window zero-padded to N [N].         */
/* ========================================================================================== */
/* n_fft the kernels transform: 512, 1024, 2048 */
int s2svc_gl_supported(int n_fft);
/* x (B, Tmax, D) -> S and X = S exp(2 pi i u).  pinv_t (nmel, bins) given: D = nmel, S = max(eps, pinv . 10^(x * scale + mean))
   (vocoder/griffin_lim.py:20-50; scale / mean [D] or both NULL); pinv_t = NULL: D = bins, S = |x * scale + mean|.
   u (B, Tmax, bins) in [0, 1) or NULL: drawn from a counter-based generator over (seed, row, frame, bin).
   X, Rprev, nsamp ([B] int32: hop * (frames - 1)) may be NULL. */
int s2svc_gl_prepare(int B, int Tmax, int nb, int D, int nmel, int hop, const float* x, const float* scale, const float* mean,
                     const float* pinv_t, float eps, const float* u, uint64_t seed, const int32_t* lens, float* S, float* X,
                     float* Rprev, int32_t* nsamp, void* stream);
/* frames[b, t] = window * irfft(X[b, t]) (the imaginary parts of bins 0 and N/2 are ignored, as numpy's irfft does) */
int s2svc_gl_synth(int B, int Tmax, int n_fft, const float* X, const int32_t* lens, const float* tables, float* frames, void* stream);
/* One iteration's second half.  R[b, t] = frame t of stft(y, center=True, zero (reflect = 0) or reflect padding), y = the overlap-add of
   `frames` over the squared-window envelope (where it exceeds FLT_MIN), trimmed by N/2: every sample is gathered from the frames that
   cover it in ascending frame order.  A = R - coef * Rprev (have_prev) or R;  X = S A / (|A| + FLT_MIN);  Rprev = R.  In place. */
int s2svc_gl_analyse(int B, int Tmax, int n_fft, int hop, int reflect, const float* frames, const float* S, const int32_t* lens,
                     const float* tables, float coef, int have_prev, float* X, float* Rprev, void* stream);
/* y (B, hop * (Tmax - 1)): the same gather, one lane per sample; zero past a row's hop * (lens[b] - 1) samples */
int s2svc_gl_ola(int B, int Tmax, int n_fft, int hop, const float* frames, const int32_t* lens, const float* tables, float* y,
                 void* stream);

/* ========================================================================================== */
/* Differentiable log-mel spectrogram and its fused L1 loss, fp32, n_fft = 1024                */
/* (csrc/melspec.hip).  replaces: urhythmic/dataset.py:23-50 (LogMelSpectrogram: reflect pad,  */
/* torchaudio MelSpectrogram(center=False, power=1), log(clamp(., 1e-5))) and the F.l1_loss    */
/* behind it in urhythmic_fine_tune_vocoder.py:191-222, forward and backward.                  */
/* Buffers: wav (B, N) fp32; mel, logmel, tgt, g_logmel (B, n_mels, T) fp32 with               */
/* T = (N + 2 pad - 1024) / hop + 1 and N > pad; partials [B T] double; frames (B, T, 1024)    */
/* fp32.  `tables` (8-byte aligned): the Griffin-Lim table for n_fft = 1024.  seg_lo / seg_len */
/* [n_mels + 1] and wud (513, 2) are the segment form of the mel basis of                      */
/* s2svc_stft_logmel_fft8, bin_seg [513] the segment of every bin.  No atomics: two calls give */
/* the same bits and a batch row equals its own B = 1 call.  LIMITS: n_mels <= 128.            */
/* ========================================================================================== */
/* 1 where the kernels apply: n_fft = 1024, win_length = n_fft, n_mels <= 128 */
int s2svc_melspec_supported(int n_fft, int win_length, int nmel);
/* mel = fb^T |STFT(reflect_pad(wav, pad))| (kept for the backward) and logmel = log(max(mel, eps)), one wavefront per frame.
   tgt given (partials too, else both NULL): partials[b T + t] = sum_m |logmel - tgt| of frame (b, t), in double. */
int s2svc_melspec_fwd(int B, int64_t Nw, int T, int hop, int pad, int nmel, const float* wav, const float* tables, const int32_t* seg_lo,
                      const int32_t* seg_len, const float* wud, float eps, float* mel, float* logmel, const float* tgt, double* partials,
                      void* stream);
/* loss[0] = fp32(inv_count * the sum of the n partials in ascending order, in double) */
int s2svc_melspec_loss_finish(int64_t n, const double* partials, double inv_count, float* loss, void* stream);
/* frames[b, t, :] = gradient of the windowed frame: the spectrum X is recomputed from wav; g_mel = g / mel where mel >= eps (0 below),
   g = g_logmel, or (g_logmel = NULL) sign(logmel - tgt) * gscale * gout[0] with sign(0) = 0; G = g_mag X / |X| (0 where |X| = 0);
   frames = window * Re sum_{k = 0 .. 512} G[k] exp(+2 pi i k n / 1024), interior bins not doubled. */
int s2svc_melspec_bwd_frames(int B, int64_t Nw, int T, int hop, int pad, int nmel, const float* wav, const float* tables, const float* wud,
                             const int32_t* bin_seg, float eps, const float* mel, const float* g_logmel, const float* logmel,
                             const float* tgt, const float* gout, float gscale, float* frames, void* stream);
/* dwav (B, N): sample j gathers the padded positions pad - j (1 <= j <= pad), j + pad and pad + 2 (N - 1) - j (N - 1 - pad <= j <= N - 2)
   from the frames that cover each, in ascending (position, frame) order, one lane per sample */
int s2svc_melspec_bwd_ola(int B, int64_t Nw, int T, int hop, int pad, const float* frames, float* dwav, void* stream);

/* ========================================================================================== */
/* Urhythmic: segmentation search and time stretcher.                                         */
/* replaces: urhythmic/segmenter.py:138-191 (_segment / _backtrack, numba-JIT on the host over */
/* a dense (T, T, K) table, and cluster_merge), urhythmic/stretcher.py:23-71 (F.interpolate    */
/* per segment + torch.cat).  LIMITS: K <= 256 units, Tmax <= 4096 frames, B <= 65535.         */
/* Frames t >= lens[b] are never read (log_probs or workspace); inputs are assumed finite.     */
/* ========================================================================================== */
/* workspace of the two launches below: max_k and argmax_k of every span's running sum, [b][end frame][start frame] */
int64_t s2svc_useg_ws_bytes(int B, int Tmax, int K);
/* log_probs (B, Tmax, K) fp32 -> ws: for 0 <= a <= e < lens[b] the fp32 running sums r_a,e[k] = r_a,e-1[k] + log_probs[e,k] (r_a,a =
   log_probs[a]; sequential, one rounding each), their maximum over k and the smallest k that attains it. */
int s2svc_useg_spans(int B, int Tmax, int K, const float* log_probs, const int32_t* lens, void* ws, void* stream);
/* The dynamic programme of _segment (the running maximum rounded to float32 after every update; gamma * s and the comparison in
   float64), the backtrack and, with labels ([K] int32 unit -> cluster; NULL: none of the last three outputs is written), cluster_merge.
   codes (B, Tmax): unit of every frame; boundaries (B, Tmax + 1): ascending from 0, nseg[b] + 1 of them; alpha (B, Tmax + 1) fp32 and
   P (B, Tmax + 1, 2) (start frame, unit) may be NULL; clusters (B, Tmax), cboundaries (B, Tmax + 1), ncl (B).  Everything past a
   row's own entries is written as zero; a row of length 0 has nseg = ncl = 0 and boundaries [0]. */
int s2svc_useg_search(int B, int Tmax, double gamma, const int32_t* lens, const void* ws, const int32_t* labels, int32_t* codes,
                      int32_t* boundaries, int32_t* nseg, float* alpha, int32_t* P, int32_t* clusters, int32_t* cboundaries,
                      int32_t* ncl, void* stream);
/* The stretch plan on the device: the merged clusters of s2svc_useg_search and the rhythm model's duration table -> the seg table
   s2svc_useg_stretch reads (Smax = Tmax).  table (n_clusters, Lmax + 1) int32: target frames of a segment of n frames of cluster c;
   INT32_MIN marks a length the rhythm model cannot map.  Per row (ncl clamped to [0, Tmax]): a segment is kept unless its cluster is
   silence_cluster and it has at most short_silence frames; a kept segment whose target is <= 0 is dropped; the survivors are written
   in order as (cboundaries[i], n, target, exclusive prefix sum of the targets), every seg row from nsegs[b] to Tmax is zero.
   status[b]: 0 ok; 1 a kept segment met INT32_MIN; 2 malformed input (n < 1, n > Lmax, cluster outside [0, n_clusters), a boundary
   outside [0, Tmax]); 3 the targets add up to more than INT32_MAX (added in 64 bits).  A row whose status is not 0 has nsegs = totals
   = 0 and an all-zero seg.  Nothing beyond ncl[b] is read and no index leaves its array whatever the tables hold.  One wave per row,
   one launch, no atomics, no workspace.
   replaces: the host work between the two (urhythmic/rhythm_model.py:150-161, two scipy calls per segment, and the two filters of
   urhythmic/stretcher.py:41-53) */
int s2svc_useg_plan(int B, int Tmax, int n_clusters, int Lmax, const int32_t* clusters /* (B, Tmax) */,
                    const int32_t* cboundaries /* (B, Tmax + 1) */, const int32_t* ncl /* (B) */,
                    const int32_t* table /* (n_clusters, Lmax + 1) */, int silence_cluster, int short_silence,
                    int32_t* seg /* (B, Tmax, 4) */, int32_t* nsegs, int32_t* totals, int32_t* status /* (B) each */, void* stream);
/* Segment-wise linear resampling (F.interpolate(mode="linear", align_corners=False) of every segment on its own, concatenated).
   x element (b, t, c) at b*sb + t*st + c*sc, t < N, dtype 0 / 1; seg (B, Smax, 4) int32 = (source start, source length, target length,
   exclusive prefix sum of the target lengths), nsegs (B); target lengths are positive.  out (B, Nmax, C) fp32, zero past the row's
   own frames.  scale > 0: the source step of every segment (1 / scale_factor, as torch uses it); otherwise source / target length. */
int s2svc_useg_stretch(int dtype, int B, int N, int C, const void* x, int64_t sb, int64_t st, int64_t sc, const int32_t* seg,
                       const int32_t* nsegs, int Smax, int Nmax, float scale, float* out, void* stream);

/* ========================================================================================== */
/* GAN losses of the HiFi-GAN fine-tuning loop (csrc/gan_loss.hip), table-driven: every tensor */
/* (pair) of a call in ONE launch.  fp32, dense tensors walked in their physical storage.      */
/* replaces: urhythmic/vocoder.py:428-465 (feature_loss, discriminator_loss, generator_loss    */
/* and their autograd: a subtract / abs or square / mean / add chain per tensor)               */
/* ========================================================================================== */
/* elements per workgroup (8192) and entries per call (64), as the library states them */
int s2svc_gan_loss_chunk(void);
int s2svc_gan_loss_max(void);
/* table (HOST, n rows of 6 int64): address of a, of b, of grad_a, of grad_b (b and the gradients may be 0), numel >= 1, kind
   (0: mean((1 - a)^2), 1: mean(a^2), 2: mean(|a - b|)).  prefix (HOST, n + 1 int32): prefix[e] = the first workgroup of entry e,
   prefix[e + 1] - prefix[e] = ceil(numel / chunk).  partials: prefix[n] doubles.  out: n + 1 floats, out[e] = fp32(the double sum of
   entry e over its numel), out[n] = fp32(the double means added in ascending order).  Two launches (chunk sums, finish), no atomics.
   replaces: urhythmic/vocoder.py:428-436 (feature_loss: kind 2 entries only) */
int s2svc_gan_feature_loss(int n, const int64_t* table /* host */, const int32_t* prefix /* host */, double* partials, float* out, void* stream);
/* One launch: t = fl(upstream[0] / numel) * sgn(a - b) with sgn(0) = 0; grad_a = t, grad_b = -t, each written where its address is not 0.
   replaces: autograd of urhythmic/vocoder.py:428-436 */
int s2svc_gan_feature_loss_bwd(int n, const int64_t* table /* host */, const int32_t* prefix /* host */, const float* upstream, void* stream);
/* The least-squares losses, kind 0 and 1 entries only, same tables and outputs.
   replaces: urhythmic/vocoder.py:439-465 (discriminator_loss, generator_loss) */
int s2svc_gan_score_loss(int n, const int64_t* table /* host */, const int32_t* prefix /* host */, double* partials, float* out, void* stream);
/* One launch: grad_a = fp32(2 upstream[0] (a - 1) / numel) (kind 0) or fp32(2 upstream[0] a / numel) (kind 1), computed in double.
   replaces: autograd of urhythmic/vocoder.py:439-465 */
int s2svc_gan_score_loss_bwd(int n, const int64_t* table /* host */, const int32_t* prefix /* host */, const float* upstream, void* stream);

/* ========================================================================================== */
/* Multi-tensor AdamW (csrc/adamw_multi.hip): up to 80 tensors per launch, their addresses as  */
/* kernel arguments.  replaces: torch.optim.AdamW.step() as urhythmic_fine_tune_vocoder.py     */
/* :99-110, :206, :222 runs it                                                                 */
/* ========================================================================================== */
/* tensors per call (80) and elements per workgroup (4096), as the library states them */
int s2svc_adamw_multi_group(void);
int s2svc_adamw_multi_chunk(void);
/* table (HOST, n rows of 4 int64): address of the parameter, of its gradient, offset of its moments in exp_avg / exp_avg_sq (a multiple
   of 4 elements, offset + numel <= moment_numel), numel.  prefix as above with the 4096-element chunk.  Per element, fp32:
   p *= decay; m += one_minus_beta1 (g - m); v = beta2 v + one_minus_beta2 g g; p -= step_size[e] * m / (sqrt(v) / bc2_sqrt[e] + eps).
   The host forms decay = 1 - lr wd, 1 - beta1 and 1 - beta2 in double (in fp32 the differences cancel) and rounds them once.
   replaces: torch.optim.AdamW.step() over the same tensors */
int s2svc_adamw_multi(int n, const int64_t* table /* host */, const int32_t* prefix /* host */, const float* step_size /* host */,
                      const float* bc2_sqrt /* host */, int64_t moment_numel, float* exp_avg, float* exp_avg_sq, float decay,
                      float one_minus_beta1, float beta2, float one_minus_beta2, float eps, void* stream);

/* ========================================================================================== */
/* Attention forward without the map (csrc/attn_flash.hip): online softmax over key tiles.     */
/* Inference only: no dropout, no backward, nothing but ctx is written.                        */
/* replaces: the scaled-dot-product core of torch.nn.MultiheadAttention inside the              */
/* nn.TransformerEncoderLayer stack of the HuBERT-Soft content encoder (urhythmic/hubert.py)   */
/* ========================================================================================== */
/* 1 if _fwd takes the problem: dtype 0 / 1, dk = 64, every row stride a whole number of 16-byte vectors and >= 64 */
int s2svc_attn_flash_supported(int dtype, int dk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo);
/* q element (b, t, h, d) at b*qbs + t*ldq + h*dk + d (t < T1), k and v alike (t < T2), ctx alike (t < T1): slices of one packed
   (B, T, 3 D) projection are such views.  16-byte aligned pointers and batch strides.  klen (B) int32 or NULL (= T2 everywhere): keys
   t >= min(klen[b], T2) are never read; query rows t >= klen[b], and every row of an utterance with klen[b] <= 0, are written as +0.
   ctx = softmax(scale * q k^T) v per (b, h), fp32 accumulation; the result of one (b, h, 64-row query tile) depends on its own
   rows and keys only -- not on B and not on T1 / T2 beyond klen[b]. */
int s2svc_attn_flash_fwd(int dtype, int B, int H, int T1, int T2, int dk, const void* q, int64_t qbs, int64_t ldq, const void* k,
                         int64_t kbs, int64_t ldk, const void* v, int64_t vbs, int64_t ldv, const int32_t* klen, float scale, void* ctx,
                         int64_t obs, int64_t ldo, void* stream);

/* ========================================================================================== */
/* HuBERT-Soft content encoder (csrc/hubert.hip): front-end layer 0 and the unit log-probs.    */
/* replaces: bshall/hubert FeatureExtractor.conv0 / norm0 / gelu, Hubert.logits, and the        */
/* log_softmax of urhythmic/model.py:33-35                                                     */
/* ========================================================================================== */
/* Conv1d(1, 512, 10, stride 5, no bias) -> GroupNorm(512, 512) -> exact GELU over wav (B, Nmax) fp32, row b being its first lens[b]
   samples padded by `pad` zeros on both sides (index arithmetic; HubertSoft.units: 40): L0_b = (lens[b] + 2 pad - 10) / 5 + 1 frames.  w (512, 10) fp32.
   _stats: per (row, channel) sum y and sum y^2 over the row's own frames in double, 32 ordered chunk pairs ws[b][32][2][512]
           (_ws_bytes(B) bytes); no atomics; samples at or beyond lens[b] are never read.
   _apply: adds the pairs in chunk order, recomputes the product, normalises with the biased variance and eps, applies gamma / beta (512)
           and the GELU, writes out (B, L0max, 512) in dtype 0 / 1; frames at or beyond L0_b are +0. */
int64_t s2svc_hubert_conv0_ws_bytes(int B);
int s2svc_hubert_conv0_stats(int B, int Nmax, int pad, const float* wav, const int32_t* lens, const float* w, double* ws, void* stream);
int s2svc_hubert_conv0_apply(int dtype, int B, int Nmax, int pad, int L0max, const float* wav, const int32_t* lens, const float* w,
                             const float* gamma, const float* beta, float eps, const double* ws, void* out, void* stream);
/* out (B * L, K) fp32 = log_softmax_k(cosine_similarity(units[row], emb[k]) / 0.1) (log_softmax = 0: the quotient itself), units (B * L, 256) in dtype 0 / 1, emb (K <= 256,
   256) fp32, cosine = x.e / (max(|x|, 1e-8) * max(|e|, 1e-8)); fp32 arithmetic, one wavefront per row.  lens (B) int32 or NULL: rows
   (b, t >= lens[b]) are written as +0. */
int s2svc_hubert_logits(int dtype, int B, int L, int K, int log_softmax, const void* units, const int32_t* lens, const float* emb, float* out,
                        void* stream);

/* ========================================================================================== */
/* Waveform conditioning (csrc/audio.hip): batched polyphase resampling and silence trimming   */
/* of padded batches with per-row lengths.  fp32, inference only, no atomics; samples at or    */
/* beyond lens[b] are never read; a batched row equals its own B = 1 call bit for bit.         */
/* replaces: torchaudio.functional.resample (urhythmic/urhythmic_resample.py:27-31),           */
/* librosa.effects.trim (urhythmic/urhythmic_convert.py:160-171, urhythmic_encode.py:122-133,  */
/* bin/preprocess.py:207-221) and the global gain of bin/preprocess.py:250                     */
/* ========================================================================================== */
/* outputs per workgroup (1024) and the floats of LDS a workgroup may stage (12288), as the library states them */
int s2svc_resample_tile(void);
int s2svc_resample_max_span(void);
/* out[b][q new + p] = sum_{k < Kb} taps[k][p] * x_b[q orig + first[p] + k - width], x_b = the first lens[b] samples of wav[b] and 0
   outside them; fp32 FMA in ascending k.  wav (B, Nmax), out (B, Mmax): outputs at or beyond out_lens[b] are +0.  taps (Kb, new_) fp32
   and first (new_) int32 with fmin <= first[p] <= fmax <= 2 width + orig (entries outside are clamped) are the banded table of
   (orig, new_) after division by their gcd.  A workgroup stages ((new_ + tile - 2) / new_) orig + fmax - fmin + Kb samples: above
   s2svc_resample_max_span() the call is refused.  One launch whatever B is. */
int s2svc_resample_poly(int B, int Nmax, int Mmax, int orig, int new_, int width, int Kb, int fmin, int fmax, const float* wav,
                        const int32_t* lens, const int32_t* out_lens, const float* taps, const int32_t* first, float* out, void* stream);
/* power[b][i] (B, nfmax) double = mean of x^2 over the centred frame [i hop - frame_length / 2, .. + frame_length) of row b, i <= lens[b] / hop
   (0 beyond); outside the row the frame reads zeros (reflect = 0) or the reflected row (reflect = 1: numpy's pad mode "reflect").
   One wavefront per frame, an ordered double sum. */
int s2svc_trim_frames(int B, int Nmax, int nfmax, int frame_length, int hop, int reflect, const float* wav, const int32_t* lens,
                      double* power, void* stream);
/* intervals (B, 2) int32 = (first hop, min(lens[b], (last + 1) hop)) over the frames i <= lens[b] / hop with
   max(amin, power[b][i]) > max(amin, max_i power[b][i]) * ratio (double), (0, 0) when there is none.  One wave per row. */
int s2svc_trim_intervals(int B, int Nmax, int nfmax, int hop, double amin, double ratio, const int32_t* lens, const double* power,
                         int32_t* intervals, void* stream);
/* out[b][i] (B, Mmax) = wav[b][start_b + i] * gain for i < end_b - start_b, +0 beyond; (start_b, end_b) = intervals[b] (device data),
   clamped to [0, Nmax]. */
int s2svc_wav_gather_rows(int B, int Nmax, int Mmax, float gain, const float* wav, const int32_t* intervals, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
